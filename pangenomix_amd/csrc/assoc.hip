// The association screen on the genome-major bitmap (reference sparse_utils.py compress_rows_spmatrix and
// ml_pipelines.py contingency_tables_from_sparse / prepare_amr_case_data): for the rows of a table restricted to a list
// of selected genomes,
//   incidence[r]   = genomes of the selection in which row r is present
//   tp[t][r]       = of those, the genomes that are set in mask t (one mask per phenotype vector)
//   block_of_row   = rows with the same set of genomes form a block; blocks are numbered by their first row
// all of it integer work: bit gathers, AND + popcount, equality of bit strings.
//
// Kernels (plain launches on one stream, no workgroup waits for another):
//   assoc_sig_kernel     one thread per row: the row's bits among the selected genomes ("signature", W = ceil(n_sel / 64)
//                        words), its popcount and a 64-bit hash. The 64 lanes of a wave are 64 neighbouring rows, so
//                        without a row map every load of the genome-major side is ONE 8-byte word for the whole wave.
//                        The image is word-major (word w of row r at sig[w * pitch + r]): every later pass is one thread
//                        per row and reads / writes whole 512-byte lines.
//   assoc_tp_kernel      grid (rows, targets): popcount(sig & mask) summed over the words; the mask words are uniform over
//                        the workgroup (scalar loads).
//   assoc_claim_kernel   open addressing in global memory (capacity = a power of two >= 2 n_rows, linear probing bounded
//                        by the capacity): a row claims an empty slot with atomicCAS or joins a slot whose owner has the
//                        same hash AND the same signature word for word, then atomicMin(first_row[slot], r). Which row
//                        owns a slot, and which slot a group of equal rows lands in, depend on the order the claims
//                        arrive in; first_row of the group's slot does not.
//   assoc_flag_kernel    rep[r] = first_row of r's slot; one ballot per wave: bit = "r is the first row of its block"
//   assoc_scan_kernel    one workgroup: exclusive prefix of the flag words' popcounts, the number of blocks
//   assoc_assign_kernel  block_of_row[r] = rank of rep[r] among the flagged rows (word prefix + popcount below its bit),
//                        rep_row[block] = its first row
// With PGX_ASSOC_DROP_EMPTY the rows without a genome in the selection take no part (block_of_row = -1): the blocks are
// those of the table after drop_empty(axis='index').
// The hash only decides where a row starts to look; a row joins a slot after its signature has been compared word for word,
// so the blocks are exact whatever the hash does (mix64 does collide on real tables: rows that differ in bit 62 of one word
// and bits 33 and 62 of the next) -- PGX_ASSOC_NARROW_HASH (a test seam) keeps 3 bits of it and must give the
// same output. Under it a row's stored hash is h & 7 (two different rows collide with probability 1/8 and the compare
// decides) and its first slot is (cap - 4 + (h & 7)) & (cap - 1): the eight start slots straddle the end of the table, so
// every table of more than four blocks wraps from slot cap - 1 to slot 0 and a chain is as long as there are blocks (the
// walk is then quadratic in the blocks).
#include "pgx_internal.h"

namespace {

constexpr int AS_THREADS = 256;
constexpr uint32_t AS_NONE = 0xFFFFFFFFu;
constexpr uint32_t AS_ERR_FULL = 1u, AS_ERR_MAP = 2u;

struct AssocGeom {
    uint32_t words, pitch, cap, flag_words;
    size_t off_sig, off_hash, off_table, off_slot, off_rep, off_flags, off_prefix, off_status, bytes;
};

AssocGeom make_geom(uint32_t n_rows, uint32_t n_sel) {
    AssocGeom g;
    g.words = std::max(1u, ceil_div_u32(n_sel, 64));
    g.pitch = ceil_div_u32(std::max(n_rows, 1u), 64) * 64;
    g.cap = 64;
    while ((uint64_t)g.cap < 2ull * n_rows) g.cap <<= 1;          // (n_rows < 2^31 / 2: checked by the callers)
    g.flag_words = g.pitch / 64;
    WsLayout ws;
    g.off_sig = ws.take((size_t)g.words * g.pitch * 8);
    g.off_hash = ws.take((size_t)g.pitch * 8);
    g.off_table = ws.take((size_t)g.cap * 8);                     // owner[cap] then first_row[cap], both filled with 0xFF
    g.off_slot = ws.take((size_t)g.pitch * 4);
    g.off_rep = ws.take((size_t)g.pitch * 4);
    g.off_flags = ws.take((size_t)g.flag_words * 8);
    g.off_prefix = ws.take((size_t)g.flag_words * 4);
    g.off_status = ws.take(16);
    g.bytes = ws.off;
    return g;
}

__device__ __forceinline__ unsigned long long mix64(unsigned long long h, unsigned long long word) {
    h = (h ^ word) * 0xff51afd7ed558ccdull;
    return h ^ (h >> 29);
}

// sig[w * pitch + r] = bit j: row r present in genome col_map[64 w + j]; inc[r] = its popcount; hash[r]. A map entry out
// of range reads nothing and raises AS_ERR_MAP.
__global__ __launch_bounds__(AS_THREADS) void assoc_sig_kernel(const unsigned long long *__restrict__ bits, uint32_t stride,
                                                               uint32_t src_rows, uint32_t n_genomes,
                                                               const int32_t *__restrict__ row_map,
                                                               const int32_t *__restrict__ col_map, uint32_t n_rows,
                                                               uint32_t n_sel, uint32_t words, uint32_t pitch,
                                                               unsigned long long *__restrict__ sig,
                                                               unsigned long long *__restrict__ hash, uint32_t *__restrict__ inc,
                                                               int narrow, uint32_t *__restrict__ status) {
    const uint32_t r = blockIdx.x * AS_THREADS + threadIdx.x;
    if (r >= n_rows) return;
    const uint32_t m = row_map ? (uint32_t)row_map[r] : r;
    const bool row_ok = m < src_rows;
    const unsigned long long *src = bits + (row_ok ? (m >> 6) : 0u);
    const uint32_t sh = m & 63u;
    unsigned long long h = 0x9e3779b97f4a7c15ull;
    uint32_t count = 0;
    bool bad = !row_ok;
    for (uint32_t w = 0; w < words; ++w) {
        unsigned long long word = 0;
        const uint32_t j1 = min(64u, n_sel - min(n_sel, w * 64u));
        for (uint32_t j = 0; j < j1; ++j) {
            const uint32_t g = col_map ? (uint32_t)col_map[w * 64u + j] : w * 64u + j;      // (uniform over the wave)
            if (g >= n_genomes) { bad = true; continue; }
            if (row_ok) word |= ((src[(size_t)g * stride] >> sh) & 1ull) << j;
        }
        sig[(size_t)w * pitch + r] = word;
        count += (uint32_t)__popcll(word);
        h = mix64(h, word);
    }
    hash[r] = narrow ? (h & 7ull) : h;                            // (uniform; PGX_ASSOC_NARROW_HASH)
    inc[r] = count;
    if (bad) atomicOr(status, AS_ERR_MAP);
}

// tp[t][r] = popcount(sig[r] & mask[t])
__global__ __launch_bounds__(AS_THREADS) void assoc_tp_kernel(const unsigned long long *__restrict__ sig,
                                                              const unsigned long long *__restrict__ masks, uint32_t n_rows,
                                                              uint32_t words, uint32_t pitch, uint32_t *__restrict__ tp) {
    const uint32_t r = blockIdx.x * AS_THREADS + threadIdx.x;
    if (r >= n_rows) return;
    const unsigned long long *mask = masks + (size_t)blockIdx.y * words;
    uint32_t count = 0;
    for (uint32_t w = 0; w < words; ++w) count += (uint32_t)__popcll(sig[(size_t)w * pitch + r] & mask[w]);
    tp[(size_t)blockIdx.y * n_rows + r] = count;
}

__global__ __launch_bounds__(AS_THREADS) void assoc_claim_kernel(const unsigned long long *__restrict__ sig,
                                                                 const unsigned long long *__restrict__ hash,
                                                                 const uint32_t *__restrict__ inc, uint32_t n_rows,
                                                                 uint32_t words, uint32_t pitch, uint32_t cap, int drop_empty,
                                                                 int narrow,
                                                                 uint32_t *__restrict__ owner, uint32_t *__restrict__ first_row,
                                                                 uint32_t *__restrict__ slot_of_row,
                                                                 uint32_t *__restrict__ status) {
    const uint32_t r = blockIdx.x * AS_THREADS + threadIdx.x;
    if (r >= n_rows) return;
    uint32_t found = AS_NONE;
    if (!(drop_empty && inc[r] == 0u)) {
        const unsigned long long h = hash[r];
        uint32_t slot = (narrow ? cap - 4u + (uint32_t)(h & 7ull) : (uint32_t)(h >> 20)) & (cap - 1u);
        for (uint32_t probe = 0; probe < cap; ++probe, slot = (slot + 1u) & (cap - 1u)) {
            uint32_t o = atomicCAS(&owner[slot], AS_NONE, r);
            if (o == AS_NONE) o = r;                              // claimed
            bool same = o == r || hash[o] == h;
            if (same && o != r)                                   // (a hash match alone is never taken as equality)
                for (uint32_t w = 0; w < words; ++w)
                    if (sig[(size_t)w * pitch + o] != sig[(size_t)w * pitch + r]) { same = false; break; }
            if (same) { found = slot; break; }
        }
        if (found == AS_NONE) atomicOr(status, AS_ERR_FULL);
        else atomicMin(&first_row[found], r);
    }
    slot_of_row[r] = found;
}

// rep[r] = the first row of r's block; flags: one bit per row, set where rep[r] == r (whole waves: every lane ballots)
__global__ __launch_bounds__(AS_THREADS) void assoc_flag_kernel(const uint32_t *__restrict__ slot_of_row,
                                                                const uint32_t *__restrict__ first_row, uint32_t n_rows,
                                                                uint32_t flag_words, uint32_t *__restrict__ rep,
                                                                unsigned long long *__restrict__ flags) {
    const uint32_t r = blockIdx.x * AS_THREADS + threadIdx.x;
    uint32_t first = AS_NONE;
    if (r < n_rows) {
        const uint32_t slot = slot_of_row[r];
        if (slot != AS_NONE) first = first_row[slot];
        rep[r] = first;
    }
    const unsigned long long word = __ballot(r < n_rows && first == r);
    if ((threadIdx.x & 63u) == 0 && (r >> 6) < flag_words) flags[r >> 6] = word;   // (the grid covers every flag word)
}

// One workgroup: prefix[i] = set bits of flags[0..i); status[1] = all of them.
__global__ __launch_bounds__(1024) void assoc_scan_kernel(const unsigned long long *__restrict__ flags, uint32_t n_words,
                                                          uint32_t *__restrict__ prefix, uint32_t *__restrict__ status) {
    __shared__ uint32_t scan[1024];
    __shared__ uint32_t base;
    if (threadIdx.x == 0) base = 0u;
    __syncthreads();
    for (uint32_t w0 = 0; w0 < n_words; w0 += 1024u) {
        const uint32_t wi = w0 + threadIdx.x;
        const uint32_t n = wi < n_words ? (uint32_t)__popcll(flags[wi]) : 0u;
        scan[threadIdx.x] = n;
        __syncthreads();
        for (uint32_t d = 1; d < 1024u; d <<= 1) {
            const uint32_t t = threadIdx.x >= d ? scan[threadIdx.x - d] : 0u;
            __syncthreads();
            scan[threadIdx.x] += t;
            __syncthreads();
        }
        if (wi < n_words) prefix[wi] = base + scan[threadIdx.x] - n;
        __syncthreads();
        if (threadIdx.x == 1023u) base += scan[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) status[1] = base;
}

__global__ __launch_bounds__(AS_THREADS) void assoc_assign_kernel(const uint32_t *__restrict__ rep,
                                                                  const unsigned long long *__restrict__ flags,
                                                                  const uint32_t *__restrict__ prefix, uint32_t n_rows,
                                                                  int32_t *__restrict__ block_of_row,
                                                                  int32_t *__restrict__ rep_row) {
    const uint32_t r = blockIdx.x * AS_THREADS + threadIdx.x;
    if (r >= n_rows) return;
    const uint32_t first = rep[r];
    if (first == AS_NONE || first >= n_rows) { block_of_row[r] = -1; return; }
    const uint32_t id = prefix[first >> 6] + (uint32_t)__popcll(flags[first >> 6] & ((1ull << (first & 63u)) - 1ull));
    block_of_row[r] = (int32_t)id;
    if (first == r && id < n_rows) rep_row[id] = (int32_t)r;
}

bool sizes_ok(uint32_t n_rows, uint32_t n_genomes, uint32_t n_sel, uint32_t n_targets) {
    return n_rows < (1u << 30) && n_genomes < (1u << 31) && n_sel < (1u << 31) && n_targets <= 65535u;
}

// Everything on the device; `stream` is synchronised (the status record is read back). d_bits: genome-major bitmap of
// src_rows rows, never written. d_row_map NULL: row r of the table is row r of the bitmap.
int assoc_run(pgx_ctx *ctx, const uint64_t *d_bits, uint32_t src_rows, uint32_t n_genomes, const int32_t *d_row_map,
              uint32_t n_rows, const int32_t *d_col_map, uint32_t n_sel, const uint64_t *d_masks, uint32_t n_targets,
              uint32_t flags, uint32_t *d_tp, uint32_t *d_inc, int32_t *d_block, int32_t *d_rep, void *d_ws, size_t ws_bytes,
              hipStream_t stream, uint32_t *out_n_blocks) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE((flags & ~(uint32_t)(PGX_ASSOC_BLOCKS | PGX_ASSOC_DROP_EMPTY | PGX_ASSOC_NARROW_HASH)) == 0, "unknown flag");
    PGX_REQUIRE(sizes_ok(n_rows, n_genomes, n_sel, n_targets), "table too large");
    PGX_REQUIRE(d_col_map || n_sel == n_genomes || n_sel == 0, "without a column map every genome is selected");
    const bool blocks = (flags & PGX_ASSOC_BLOCKS) != 0;
    const int narrow = (flags & PGX_ASSOC_NARROW_HASH) != 0;
    if (out_n_blocks) *out_n_blocks = 0;
    if (n_rows == 0) return PGX_OK;
    PGX_REQUIRE(d_bits && d_ws && d_inc, "NULL argument");
    PGX_REQUIRE(n_targets == 0 || (d_masks && d_tp), "NULL argument");
    PGX_REQUIRE(!blocks || (d_block && d_rep && out_n_blocks), "NULL argument");
    const AssocGeom g = make_geom(n_rows, n_sel);
    PGX_REQUIRE(ws_bytes >= g.bytes, "workspace too small (see pgx_assoc_workspace_bytes)");
    PGX_REQUIRE(((uintptr_t)d_ws & 15u) == 0, "workspace must be 16-byte aligned");
    HostVec<uint32_t> h_status(ctx, AS_HOST_STATUS, 4);
    if (!h_status.ok()) { pgx_set_error("%s: out of page-locked host memory", __func__); return PGX_ERR_NOMEM; }
    char *p = (char *)d_ws;
    unsigned long long *sig = (unsigned long long *)(p + g.off_sig), *hash = (unsigned long long *)(p + g.off_hash);
    uint32_t *owner = (uint32_t *)(p + g.off_table), *first_row = owner + g.cap;
    uint32_t *slot_of_row = (uint32_t *)(p + g.off_slot), *rep = (uint32_t *)(p + g.off_rep);
    unsigned long long *flagw = (unsigned long long *)(p + g.off_flags);
    uint32_t *prefix = (uint32_t *)(p + g.off_prefix), *status = (uint32_t *)(p + g.off_status);
    const uint32_t stride = pgx_bitmap_stride_words(src_rows);
    const uint32_t row_blocks = ceil_div_u32(n_rows, AS_THREADS);

    PGX_HIP(hipMemsetAsync(status, 0, 16, stream));
    {
        ProfScope prof(ctx, "assoc_sig_kernel", stream);
        assoc_sig_kernel<<<row_blocks, AS_THREADS, 0, stream>>>((const unsigned long long *)d_bits, stride, src_rows, n_genomes,
                                                                d_row_map, d_col_map, n_rows, n_sel, g.words, g.pitch, sig, hash,
                                                                d_inc, narrow, status);
    }
    PGX_HIP(hipGetLastError());
    if (n_targets) {
        ProfScope prof(ctx, "assoc_tp_kernel", stream);
        assoc_tp_kernel<<<dim3(row_blocks, n_targets), AS_THREADS, 0, stream>>>(sig, (const unsigned long long *)d_masks, n_rows,
                                                                               g.words, g.pitch, d_tp);
        PGX_HIP(hipGetLastError());
    }
    if (blocks) {
        PGX_HIP(hipMemsetAsync(owner, 0xFF, (size_t)g.cap * 8, stream));
        {
            ProfScope prof(ctx, "assoc_claim_kernel", stream);
            assoc_claim_kernel<<<row_blocks, AS_THREADS, 0, stream>>>(sig, hash, d_inc, n_rows, g.words, g.pitch, g.cap,
                                                                      (flags & PGX_ASSOC_DROP_EMPTY) != 0, narrow, owner,
                                                                      first_row, slot_of_row, status);
        }
        PGX_HIP(hipGetLastError());
        {
            ProfScope prof(ctx, "assoc_flag_kernel", stream);
            assoc_flag_kernel<<<ceil_div_u32(g.pitch, AS_THREADS), AS_THREADS, 0, stream>>>(slot_of_row, first_row, n_rows,
                                                                                           g.flag_words, rep, flagw);
        }
        PGX_HIP(hipGetLastError());
        {
            ProfScope prof(ctx, "assoc_scan_kernel", stream);
            assoc_scan_kernel<<<1, 1024, 0, stream>>>(flagw, g.flag_words, prefix, status);
        }
        PGX_HIP(hipGetLastError());
        {
            ProfScope prof(ctx, "assoc_assign_kernel", stream);
            assoc_assign_kernel<<<row_blocks, AS_THREADS, 0, stream>>>(rep, flagw, prefix, n_rows, d_block, d_rep);
        }
        PGX_HIP(hipGetLastError());
    }
    PGX_HIP(hipMemcpyAsync(h_status.data(), status, 8, hipMemcpyDeviceToHost, stream));
    PGX_HIP(hipStreamSynchronize(stream));
    PGX_REQUIRE(!(h_status[0] & AS_ERR_MAP), "row or column map entry out of range");
    if (h_status[0] & AS_ERR_FULL) {
        pgx_set_error("%s: the block table is full", __func__);
        return PGX_ERR_INTERNAL;
    }
    if (blocks) {
        PGX_REQUIRE(h_status[1] <= n_rows, "inconsistent block count");
        *out_n_blocks = h_status[1];
    }
    return PGX_OK;
}

// maps and masks up, assoc_run on the context's buffers, results down
int assoc_staged(pgx_ctx *ctx, const uint64_t *d_bits, uint32_t src_rows, uint32_t n_genomes, const int32_t *row_map,
                 uint32_t n_rows, const int32_t *col_map, uint32_t n_sel, const uint64_t *masks, uint32_t n_targets,
                 uint32_t flags, uint32_t *out_tp, uint32_t *out_inc, int32_t *out_block, int32_t *out_rep,
                 uint32_t *out_n_blocks) {
    const bool blocks = (flags & PGX_ASSOC_BLOCKS) != 0;
    PGX_REQUIRE(out_inc || n_rows == 0, "NULL argument");
    PGX_REQUIRE(n_targets == 0 || n_rows == 0 || (masks && out_tp), "NULL argument");
    PGX_REQUIRE(!blocks || (out_n_blocks && (n_rows == 0 || (out_block && out_rep))), "NULL argument");
    PGX_REQUIRE(col_map || n_sel == n_genomes || n_sel == 0, "without a column map every genome is selected");
    for (uint32_t j = 0; col_map && j < n_sel; ++j)
        PGX_REQUIRE(col_map[j] >= 0 && (uint32_t)col_map[j] < n_genomes, "column map entry out of range");
    for (uint32_t i = 0; row_map && i < n_rows; ++i)
        PGX_REQUIRE(row_map[i] >= 0 && (uint32_t)row_map[i] < src_rows, "row map entry out of range");
    if (out_n_blocks) *out_n_blocks = 0;
    if (n_rows == 0) return PGX_OK;
    hipStream_t stream = ctx->stream;
    const AssocGeom g = make_geom(n_rows, n_sel);
    DevBuf d_ws(ctx, AS_SLOT_WS);
    DevPack in(ctx, AS_SLOT_IN), res(ctx, AS_SLOT_OUT);
    const PackPart rmap = in.in(row_map, n_rows), cmap = in.in(col_map, n_sel),
                   target_masks = in.in(masks, (size_t)n_targets * g.words);
    // block_of_row comes down only with PGX_ASSOC_BLOCKS, rep_row as far as there are blocks (below)
    const PackPart inc = res.out(out_inc, n_rows), tp = res.out(out_tp, (size_t)n_targets * n_rows),
                   block = res.out(blocks ? out_block : nullptr, n_rows), rep = res.out<int32_t>(nullptr, n_rows);
    PGX_HIP(d_ws.alloc(g.bytes));
    PGX_HIP(in.alloc());
    PGX_HIP(res.alloc());
    PGX_HIP(in.upload(stream));
    uint32_t n_blocks = 0;
    const int rc = assoc_run(ctx, d_bits, src_rows, n_genomes, in.dev_if(row_map, rmap), n_rows,
                             in.dev_if(col_map, cmap), n_sel, in.dev<uint64_t>(target_masks), n_targets, flags,
                             res.dev<uint32_t>(tp), res.dev<uint32_t>(inc), res.dev<int32_t>(block), res.dev<int32_t>(rep),
                             d_ws.p, g.bytes, stream, &n_blocks);
    if (rc != PGX_OK) return rc;
    PGX_HIP(res.download(stream));
    if (blocks) {
        PGX_HIP(res.download(rep, 0, n_blocks, out_rep, stream));
        *out_n_blocks = n_blocks;
    }
    PGX_HIP(hipStreamSynchronize(stream));
    return PGX_OK;
}

int assoc_host(pgx_ctx *ctx, const int32_t *rows, const int32_t *genomes, uint64_t n_records, uint32_t n_rows,
               uint32_t n_genomes, const int32_t *col_map, uint32_t n_sel, const uint64_t *masks, uint32_t n_targets,
               uint32_t flags, uint32_t *out_tp, uint32_t *out_inc, int32_t *out_block, int32_t *out_rep,
               uint32_t *out_n_blocks, uint64_t *out_duplicates) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(n_records == 0 || (rows && genomes), "NULL record arrays");
    PGX_REQUIRE(sizes_ok(n_rows, n_genomes, n_sel, n_targets), "table too large");
    PGX_HIP(hipSetDevice(ctx->device_id));
    DevBuf d_bits(ctx, AS_SLOT_BITS), d_cnt(ctx, AS_SLOT_CNT);
    uint64_t dup = 0;
    const int rc = pgx_load_coo_bitmap(ctx, rows, genomes, n_records, n_rows, n_genomes, AS_SLOT_ROWS, AS_SLOT_GENOMES, d_bits,
                                       d_cnt, &dup);
    if (rc != PGX_OK) return rc;
    if (out_duplicates) *out_duplicates = dup;
    if (out_n_blocks) *out_n_blocks = 0;
    if (dup) return PGX_OK;                   // not a 0/1 table: nothing is computed
    return assoc_staged(ctx, d_bits.as<uint64_t>(), n_rows, n_genomes, nullptr, n_rows, col_map, n_sel, masks, n_targets, flags,
                        out_tp, out_inc, out_block, out_rep, out_n_blocks);
}

int assoc_resident(pgx_ctx *ctx, uint64_t token, const int32_t *row_map, uint32_t n_rows, uint32_t n_genomes,
                   const int32_t *col_map, uint32_t n_sel, const uint64_t *masks, uint32_t n_targets, uint32_t flags,
                   uint32_t *out_tp, uint32_t *out_inc, int32_t *out_block, int32_t *out_rep, uint32_t *out_n_blocks) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(n_rows == 0 || row_map, "NULL row map");
    ResidentBitmap src;
    const int rc = pgx_resident_bitmap(ctx, token, n_genomes, &src);
    if (rc != PGX_OK) return rc;
    PGX_REQUIRE(sizes_ok(n_rows, n_genomes, n_sel, n_targets), "table too large");
    PGX_HIP(hipSetDevice(ctx->device_id));
    return assoc_staged(ctx, src.d_bits, src.n_genes, n_genomes, row_map, n_rows, col_map, n_sel, masks, n_targets, flags,
                        out_tp, out_inc, out_block, out_rep, out_n_blocks);
}

}  // namespace

extern "C" {

size_t pgx_assoc_workspace_bytes(uint32_t n_rows, uint32_t n_selected) {
    if (!sizes_ok(n_rows, 0, n_selected, 0)) return 0;
    return make_geom(n_rows, n_selected).bytes;
}

int pgx_assoc(pgx_ctx *ctx, const int32_t *rows, const int32_t *genomes, uint64_t n_records, uint32_t n_rows,
              uint32_t n_genomes, const int32_t *col_map, uint32_t n_selected, const uint64_t *masks, uint32_t n_targets,
              uint32_t flags, uint32_t *out_tp, uint32_t *out_incidence, int32_t *out_block_of_row, int32_t *out_rep_row,
              uint32_t *out_n_blocks, uint64_t *out_duplicates) {
    return guarded(__func__, [&] {
        return assoc_host(ctx, rows, genomes, n_records, n_rows, n_genomes, col_map, n_selected, masks, n_targets, flags,
                          out_tp, out_incidence, out_block_of_row, out_rep_row, out_n_blocks, out_duplicates);
    });
}

int pgx_assoc_resident(pgx_ctx *ctx, uint64_t token, const int32_t *row_map, uint32_t n_rows, uint32_t n_genomes,
                       const int32_t *col_map, uint32_t n_selected, const uint64_t *masks, uint32_t n_targets, uint32_t flags,
                       uint32_t *out_tp, uint32_t *out_incidence, int32_t *out_block_of_row, int32_t *out_rep_row,
                       uint32_t *out_n_blocks) {
    return guarded(__func__, [&] {
        return assoc_resident(ctx, token, row_map, n_rows, n_genomes, col_map, n_selected, masks, n_targets, flags, out_tp,
                              out_incidence, out_block_of_row, out_rep_row, out_n_blocks);
    });
}

int pgx_assoc_dev(pgx_ctx *ctx, const uint64_t *d_bits, uint32_t n_rows, uint32_t n_genomes, const int32_t *d_col_map,
                  uint32_t n_selected, const uint64_t *d_masks, uint32_t n_targets, uint32_t flags, uint32_t *d_tp,
                  uint32_t *d_incidence, int32_t *d_block_of_row, int32_t *d_rep_row, void *d_workspace,
                  size_t workspace_bytes, void *stream, uint32_t *out_n_blocks) {
    return guarded(__func__, [&] {
        return assoc_run(ctx, d_bits, n_rows, n_genomes, nullptr, n_rows, d_col_map, n_selected, d_masks, n_targets, flags,
                         d_tp, d_incidence, d_block_of_row, d_rep_row, d_workspace, workspace_bytes, (hipStream_t)stream,
                         out_n_blocks);
    });
}

}  // extern "C"
