// Comparison of two concept lists (reference fcd.py:168-196, compute_concept_list_similarity): every concept of F1, in
// order, takes the unmatched concept of F2 it shares the most cells with, the lowest index among equals.
//
// A concept is a row bit mask (stride_r words) and a column bit mask (stride_c words), so an index listed twice counts
// once, as in the reference's sets. The cells two concepts share are
//     O[i][j] = popcount(rows1[i] & rows2[j]) * popcount(cols1[i] & cols2[j])
// a binary matrix product. The n1 x n2 matrix never has to exist: F1 is walked in blocks of FM_RB concepts, and per block
//   fcd_lists_to_masks_kernel   (host entry only) the block's lists -> masks, one launch per family, atomicOr per element
//   fcd_overlap_kernel          one workgroup per 32 x 32 tile of pairs, 2 x 2 pairs per thread, both operands staged
//                               in LDS in chunks of 512 bytes per mask; every output word has one writer, no atomics
//   fcd_match_kernel            ONE workgroup: per concept of the block an arg max over the unmatched j (largest value,
//                               lowest j among equals -- a total order, so the result does not depend on the lanes'
//                               order), one __syncthreads() per concept; the owner thread of j retires it
// run in stream order without a synchronisation in between. No workgroup waits for another.
#include <vector>

#include "pgx_internal.h"

namespace {

constexpr int FM_THREADS = 256;
constexpr uint32_t FM_TILE = 32;               // concepts of either family per workgroup of the overlap kernel
constexpr uint32_t FM_CHUNK = 32;              // 16-byte lanes of a mask per LDS chunk (512 bytes)
// LDS row pitch in 16-byte lanes: 33 lanes = 132 dwords = 4 banks more than a multiple of the 64 banks. The 16 lanes a
// ds_read_b128 serves at once read 16 consecutive rows (mod 16) of one operand, which then start 4 banks apart and cover
// all 64 banks once, and 2 rows of the other operand, 4 banks apart as well; lanes with the same row broadcast.
constexpr uint32_t FM_PITCH = FM_CHUNK + 1;
constexpr uint32_t FM_RB = 256;                // concepts of F1 per block
constexpr int FM_MATCH_THREADS = 1024;
constexpr int FM_MATCH_WAVES = FM_MATCH_THREADS / 64;

struct MatchGeom {
    uint32_t stride_r, stride_c;
    size_t off_o, off_flags, off_m2r, off_m2c, off_m1r, off_m1c, bytes;
};

MatchGeom match_geom(uint32_t n_rows, uint32_t n_cols, uint64_t n2) {
    MatchGeom g;
    g.stride_r = pgx_bitmap_stride_words(n_rows);
    g.stride_c = pgx_bitmap_stride_words(n_cols);
    WsLayout ws;
    g.off_m2r = ws.take((size_t)n2 * g.stride_r * 8);          // masks of F2
    g.off_m2c = ws.take((size_t)n2 * g.stride_c * 8);
    g.off_m1r = ws.take((size_t)FM_RB * g.stride_r * 8);       // masks of one block of F1
    g.off_m1c = ws.take((size_t)FM_RB * g.stride_c * 8);
    g.off_o = ws.take((size_t)FM_RB * n2 * 8);                 // one block of O
    g.off_flags = ws.take((size_t)n2);                         // unmatched flags, one byte per concept of F2
    g.bytes = ws.off;                                          // (the result record is the caller's total itself)
    return g;
}

// the sizes every entry takes: 0 = fine
const char *match_sizes_bad(uint64_t n_rows, uint64_t n_cols, uint64_t n1, uint64_t n2) {
    const uint64_t lim = 1ull << 31;
    if (n_rows >= lim || n_cols >= lim) return "table too large";
    if (n1 >= lim || n2 >= lim) return "too many concepts";
    const unsigned __int128 cells = (unsigned __int128)n_rows * n_cols * std::min(n1, n2);
    if (cells >> 63) return "the total overlap could exceed 63 bits";
    return nullptr;
}

__device__ __forceinline__ uint32_t popc_and128(const uint4 &a, const uint4 &b) {
    return __popc(a.x & b.x) + __popc(a.y & b.y) + __popc(a.z & b.z) + __popc(a.w & b.w);
}

// masks[(c - c0) * stride ...] |= the bits of the elements idx[off[c0] .. off[c0 + nc)) of concepts c0 .. c0 + nc: an
// element finds its concept by a search in the offsets (empty concepts own no element). The indices are checked on the
// host; masks are zero before the launch.
__global__ __launch_bounds__(FM_THREADS) void fcd_lists_to_masks_kernel(const int32_t *__restrict__ idx,
                                                                        const uint64_t *__restrict__ off, uint32_t c0,
                                                                        uint32_t nc, uint32_t stride,
                                                                        unsigned long long *__restrict__ masks) {
    const uint64_t e1 = off[c0 + nc];
    for (uint64_t e = off[c0] + (uint64_t)blockIdx.x * FM_THREADS + threadIdx.x; e < e1; e += (uint64_t)gridDim.x * FM_THREADS) {
        uint32_t lo = c0, hi = c0 + nc;                    // off[lo] <= e < off[hi]
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (off[mid] <= e) lo = mid; else hi = mid;
        }
        const uint32_t r = (uint32_t)idx[e];
        atomicOr(&masks[(size_t)(lo - c0) * stride + (r >> 6)], 1ull << (r & 63u));
    }
}

// c<a><b> += popcount(A[ti + 16 a] & B[tj + 16 b]) over masks of `lanes` 16-byte lanes; A, B: the tile's first masks,
// nA, nB of them exist (the others count as empty)
__device__ __forceinline__ void tile_counts(const uint4 *__restrict__ A, const uint4 *__restrict__ B, uint32_t lanes,
                                            uint32_t nA, uint32_t nB, uint4 (*sA)[FM_PITCH], uint4 (*sB)[FM_PITCH],
                                            uint32_t &c00, uint32_t &c01, uint32_t &c10, uint32_t &c11) {
    const uint32_t ti = threadIdx.x >> 4, tj = threadIdx.x & 15u;
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    for (uint32_t l0 = 0; l0 < lanes; l0 += FM_CHUNK) {
        const uint32_t w = min(FM_CHUNK, lanes - l0);     // (a multiple of 8: the stride is a multiple of 128 bytes)
        __syncthreads();                                  // the chunk before has been read
        for (uint32_t e = threadIdx.x; e < FM_TILE * FM_CHUNK; e += FM_THREADS) {
            const uint32_t r = e / FM_CHUNK, l = e % FM_CHUNK;
            if (l < w) {
                uint4 va = zero, vb = zero;
                if (r < nA) va = A[(size_t)r * lanes + l0 + l];
                if (r < nB) vb = B[(size_t)r * lanes + l0 + l];
                sA[r][l] = va;
                sB[r][l] = vb;
            }
        }
        __syncthreads();
#pragma unroll 4
        for (uint32_t l = 0; l < w; ++l) {
            const uint4 a0 = sA[ti][l], a1 = sA[ti + 16u][l], b0 = sB[tj][l], b1 = sB[tj + 16u][l];
            c00 += popc_and128(a0, b0);
            c01 += popc_and128(a0, b1);
            c10 += popc_and128(a1, b0);
            c11 += popc_and128(a1, b1);
        }
    }
}

// O[i][j] = popcount(r1[i] & r2[j]) * popcount(c1[i] & c2[j]) for i < nb, j < n2; O has n2 words per row. Workgroup
// (blockIdx.x, blockIdx.y) owns the tile of 32 j x 32 i. Counts are exact in 32 bits (fewer than 2^31 rows / columns).
__global__ __launch_bounds__(FM_THREADS) void fcd_overlap_kernel(const uint4 *__restrict__ r1, const uint4 *__restrict__ c1,
                                                                 uint32_t nb, const uint4 *__restrict__ r2,
                                                                 const uint4 *__restrict__ c2, uint32_t n2, uint32_t lanes_r,
                                                                 uint32_t lanes_c, unsigned long long *__restrict__ O) {
    __shared__ uint4 sA[FM_TILE][FM_PITCH];
    __shared__ uint4 sB[FM_TILE][FM_PITCH];
    const uint32_t i0 = blockIdx.y * FM_TILE, j0 = blockIdx.x * FM_TILE;
    const uint32_t nA = min(FM_TILE, nb - i0), nB = min(FM_TILE, n2 - j0);
    uint32_t r00 = 0u, r01 = 0u, r10 = 0u, r11 = 0u, k00 = 0u, k01 = 0u, k10 = 0u, k11 = 0u;
    tile_counts(r1 + (size_t)i0 * lanes_r, r2 + (size_t)j0 * lanes_r, lanes_r, nA, nB, sA, sB, r00, r01, r10, r11);
    tile_counts(c1 + (size_t)i0 * lanes_c, c2 + (size_t)j0 * lanes_c, lanes_c, nA, nB, sA, sB, k00, k01, k10, k11);
    const uint32_t ti = threadIdx.x >> 4, tj = threadIdx.x & 15u;
    unsigned long long *out = O + (size_t)(i0 + ti) * n2 + j0 + tj;      // (formed only: stored where the pair exists)
    if (ti < nA && tj < nB) out[0] = (unsigned long long)r00 * k00;
    if (ti < nA && tj + 16u < nB) out[16] = (unsigned long long)r01 * k01;
    if (ti + 16u < nA && tj < nB) out[(size_t)16 * n2] = (unsigned long long)r10 * k10;
    if (ti + 16u < nA && tj + 16u < nB) out[(size_t)16 * n2 + 16] = (unsigned long long)r11 * k11;
}

// is (a, ia) to be preferred to (b, ib)? The larger value, the lower index among equals; an index of -1 is no candidate.
__device__ __forceinline__ bool match_better(unsigned long long a, int ia, unsigned long long b, int ib) {
    if (ia < 0) return false;
    if (ib < 0) return true;
    return a > b || (a == b && ia < ib);
}

// ONE workgroup. For s = 0 .. n_steps: concept i_first + s of F1 (row s of O) takes the unmatched j with the largest
// O[s][j], the lowest j among equals; match / overlap [i_first + s] = (j, O[s][j]); j is retired; *total (0 when `first`)
// += O[s][j]. Thread t owns the flags of the j with j % 1024 == t: it alone reads them and it alone clears them, so a
// flag never travels between threads. The caller keeps n_steps <= the number of unmatched j.
__global__ __launch_bounds__(FM_MATCH_THREADS) void fcd_match_kernel(const unsigned long long *__restrict__ O, uint32_t n2,
                                                                     uint32_t i_first, uint32_t n_steps,
                                                                     uint8_t *unmatched, long long *__restrict__ match,
                                                                     unsigned long long *__restrict__ overlap,
                                                                     unsigned long long *__restrict__ total, int first) {
    __shared__ unsigned long long s_val[2][FM_MATCH_WAVES];
    __shared__ int s_idx[2][FM_MATCH_WAVES];
    unsigned long long sum = 0ull;
    if (threadIdx.x == 0 && !first) sum = *total;
    for (uint32_t s = 0; s < n_steps; ++s) {
        const unsigned long long *row = O + (size_t)s * n2;
        unsigned long long bv = 0ull;
        int bi = -1;
        for (uint32_t j = threadIdx.x; j < n2; j += FM_MATCH_THREADS) {   // ascending: a thread keeps its first maximum
            if (!unmatched[j]) continue;
            const unsigned long long v = row[j];
            if (bi < 0 || v > bv) { bv = v; bi = (int)j; }
        }
        for (int d = 32; d > 0; d >>= 1) {                // (both lanes of a pair pick the same one: the order is total)
            const unsigned long long ov = __shfl_xor(bv, d);
            const int oi = __shfl_xor(bi, d);
            if (match_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        const uint32_t buf = s & 1u;     // two buffers: a wave may write step s + 1 while another still reads step s
        if ((threadIdx.x & 63u) == 0) { s_val[buf][threadIdx.x >> 6] = bv; s_idx[buf][threadIdx.x >> 6] = bi; }
        __syncthreads();
        bv = s_val[buf][0]; bi = s_idx[buf][0];
#pragma unroll
        for (int w = 1; w < FM_MATCH_WAVES; ++w)
            if (match_better(s_val[buf][w], s_idx[buf][w], bv, bi)) { bv = s_val[buf][w]; bi = s_idx[buf][w]; }
        if (bi >= 0 && ((uint32_t)bi % FM_MATCH_THREADS) == threadIdx.x) unmatched[bi] = 0;
        if (threadIdx.x == 0) {
            match[i_first + s] = bi;
            overlap[i_first + s] = bi >= 0 ? bv : 0ull;
            sum += bi >= 0 ? bv : 0ull;
        }
    }
    if (threadIdx.x == 0) *total = sum;
}

// The block loop on masks F2 (m2r, m2c) that exist already. prep(b0, nb, &m1r, &m1c): the masks of concepts b0 .. b0 + nb
// of F1, enqueued on `stream`. O of a block goes into d_matrix (all n1 rows are then computed) or else into d_oblock.
template <typename Prep>
int match_blocks(pgx_ctx *ctx, uint32_t n1, uint32_t n2, const MatchGeom &g, const unsigned long long *m2r,
                 const unsigned long long *m2c, long long *d_match, unsigned long long *d_overlap, unsigned long long *d_total,
                 unsigned long long *d_matrix, unsigned long long *d_oblock, uint8_t *d_flags, hipStream_t stream, Prep prep) {
    const uint32_t k = std::min(n1, n2), n_compute = d_matrix ? n1 : k;
    PGX_HIP(hipMemsetAsync(d_flags, 1, n2, stream));
    for (uint32_t b0 = 0; b0 < n_compute; b0 += FM_RB) {
        const uint32_t nb = std::min(FM_RB, n_compute - b0);
        const unsigned long long *m1r = nullptr, *m1c = nullptr;
        const int rc = prep(b0, nb, &m1r, &m1c);
        if (rc != PGX_OK) return rc;
        unsigned long long *O = d_matrix ? d_matrix + (size_t)b0 * n2 : d_oblock;
        {
            ProfScope prof(ctx, "fcd_overlap_kernel", stream);
            fcd_overlap_kernel<<<dim3(ceil_div_u32(n2, FM_TILE), ceil_div_u32(nb, FM_TILE)), FM_THREADS, 0, stream>>>(
                (const uint4 *)m1r, (const uint4 *)m1c, nb, (const uint4 *)m2r, (const uint4 *)m2c, n2, g.stride_r / 2,
                g.stride_c / 2, O);
        }
        PGX_HIP(hipGetLastError());
        if (b0 < k) {
            ProfScope prof(ctx, "fcd_match_kernel", stream);
            fcd_match_kernel<<<1, FM_MATCH_THREADS, 0, stream>>>(O, n2, b0, std::min(nb, k - b0), d_flags, d_match, d_overlap,
                                                                 d_total, b0 == 0);
        }
        PGX_HIP(hipGetLastError());
    }
    return PGX_OK;
}

int match_dev(pgx_ctx *ctx, const uint64_t *d_row_masks1, const uint64_t *d_col_masks1, uint64_t n1,
              const uint64_t *d_row_masks2, const uint64_t *d_col_masks2, uint64_t n2, uint32_t n_rows, uint32_t n_cols,
              int64_t *d_match, uint64_t *d_overlap, uint64_t *d_total, uint64_t *d_matrix, void *d_ws, size_t ws_bytes,
              hipStream_t stream) {
    PGX_REQUIRE(ctx && d_total, "NULL argument");
    const char *bad = match_sizes_bad(n_rows, n_cols, n1, n2);
    PGX_REQUIRE(!bad, bad);
    PGX_REQUIRE(((uintptr_t)d_total & 7u) == 0, "d_total must be 8-byte aligned");
    if (n1 == 0 || n2 == 0) {                              // nothing to pair and an empty matrix: no launch
        PGX_HIP(hipMemsetAsync(d_total, 0, 8, stream));
        return PGX_OK;
    }
    PGX_REQUIRE(d_row_masks1 && d_col_masks1 && d_row_masks2 && d_col_masks2 && d_match && d_overlap && d_ws, "NULL argument");
    PGX_REQUIRE((((uintptr_t)d_row_masks1 | (uintptr_t)d_col_masks1 | (uintptr_t)d_row_masks2 | (uintptr_t)d_col_masks2 |
                  (uintptr_t)d_ws) & 15u) == 0, "masks and workspace must be 16-byte aligned");
    PGX_REQUIRE((((uintptr_t)d_match | (uintptr_t)d_overlap | (uintptr_t)d_matrix) & 7u) == 0, "outputs must be 8-byte aligned");
    const MatchGeom g = match_geom(n_rows, n_cols, n2);
    PGX_REQUIRE(ws_bytes >= g.bytes, "workspace too small (see pgx_fcd_match_workspace_bytes)");
    char *p = (char *)d_ws;
    const unsigned long long *r1 = (const unsigned long long *)d_row_masks1, *c1 = (const unsigned long long *)d_col_masks1;
    return match_blocks(ctx, (uint32_t)n1, (uint32_t)n2, g, (const unsigned long long *)d_row_masks2,
                        (const unsigned long long *)d_col_masks2, (long long *)d_match, (unsigned long long *)d_overlap,
                        (unsigned long long *)d_total, (unsigned long long *)d_matrix, (unsigned long long *)(p + g.off_o),
                        (uint8_t *)(p + g.off_flags), stream,
                        [&](uint32_t b0, uint32_t, const unsigned long long **m1r, const unsigned long long **m1c) {
                            *m1r = r1 + (size_t)b0 * g.stride_r;
                            *m1c = c1 + (size_t)b0 * g.stride_c;
                            return (int)PGX_OK;
                        });
}

// one family's lists as the host hands them over: checked here, then uploaded
struct HostLists {
    const int32_t *idx;
    const uint64_t *off;
    uint64_t n, bound;
    const char *what;
};

int check_lists(const HostLists &L, uint64_t *n_entries) {
    *n_entries = 0;
    if (L.n == 0) return PGX_OK;
    PGX_REQUIRE(L.off, "NULL offsets");
    const uint64_t total = L.off[L.n];
    PGX_REQUIRE(L.off[0] == 0 && (total == 0 || L.idx), "concept offsets must start at 0 over an index array");
    for (uint64_t i = 0; i < L.n; ++i)
        PGX_REQUIRE(L.off[i] <= L.off[i + 1] && L.off[i + 1] <= total, "concept offsets out of order");
    for (uint64_t e = 0; e < total; ++e)
        if (L.idx[e] < 0 || (uint64_t)L.idx[e] >= L.bound) {
            pgx_set_error("%s: concept %s out of range", __func__, L.what);
            return PGX_ERR_INVALID;
        }
    *n_entries = total;
    return PGX_OK;
}

int launch_masks(pgx_ctx *ctx, const int32_t *d_idx, const uint64_t *d_off, const uint64_t *h_off, uint32_t c0, uint32_t nc,
                 uint32_t stride, unsigned long long *d_masks, hipStream_t stream) {
    PGX_HIP(hipMemsetAsync(d_masks, 0, (size_t)nc * stride * 8, stream));
    const uint64_t n = h_off[c0 + nc] - h_off[c0];
    if (n == 0) return PGX_OK;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + FM_THREADS - 1) / FM_THREADS, 1u << 20);
    {
        ProfScope prof(ctx, "fcd_lists_to_masks_kernel", stream);
        fcd_lists_to_masks_kernel<<<blocks, FM_THREADS, 0, stream>>>(d_idx, d_off, c0, nc, stride, d_masks);
    }
    PGX_HIP(hipGetLastError());
    return PGX_OK;
}

int match_host(pgx_ctx *ctx, uint32_t n_rows, uint32_t n_cols, const int32_t *rows1, const uint64_t *row_off1,
               const int32_t *cols1, const uint64_t *col_off1, uint64_t n1, const int32_t *rows2, const uint64_t *row_off2,
               const int32_t *cols2, const uint64_t *col_off2, uint64_t n2, int64_t *out_match, uint64_t *out_overlap,
               uint64_t *out_total, uint64_t *out_matrix) {
    PGX_REQUIRE(ctx && out_total, "NULL argument");
    const char *bad = match_sizes_bad(n_rows, n_cols, n1, n2);
    PGX_REQUIRE(!bad, bad);
    const HostLists L[4] = {{rows1, row_off1, n1, n_rows, "row"}, {cols1, col_off1, n1, n_cols, "column"},
                            {rows2, row_off2, n2, n_rows, "row"}, {cols2, col_off2, n2, n_cols, "column"}};
    uint64_t ne[4];
    for (int f = 0; f < 4; ++f) {
        const int rc = check_lists(L[f], &ne[f]);
        if (rc != PGX_OK) return rc;
    }
    *out_total = 0;
    if (n1 == 0 || n2 == 0) return PGX_OK;
    const uint64_t k = std::min(n1, n2);
    PGX_REQUIRE(out_match && out_overlap, "NULL argument");
    PGX_HIP(hipSetDevice(ctx->device_id));
    hipStream_t stream = ctx->stream;
    const MatchGeom g = match_geom(n_rows, n_cols, n2);
    DevBuf d_ws(ctx, FC_SLOT_M_WS);
    DevPack lists(ctx, FC_SLOT_M_LISTS), res(ctx, FC_SLOT_M_OUT), mat(ctx, FC_SLOT_M_MATRIX);
    PackPart idx[4], off[4];
    for (int f = 0; f < 4; ++f) {
        idx[f] = lists.in(L[f].idx, ne[f]);
        off[f] = lists.in(L[f].off, L[f].n + 1);
    }
    const PackPart r_match = res.out(out_match, k), r_overlap = res.out(out_overlap, k), r_total = res.out(out_total, 1);
    PGX_HIP(lists.alloc());
    PGX_HIP(d_ws.alloc(g.bytes));
    PGX_HIP(res.alloc());
    const PackPart r_matrix = mat.out(out_matrix, out_matrix ? (size_t)n1 * n2 : 0);
    if (out_matrix) PGX_HIP(mat.alloc());                  // (its slot is not touched otherwise)
    PGX_HIP(lists.upload(stream));
    char *pw = d_ws.as<char>();
    const int32_t *d_idx[4];
    const uint64_t *d_off[4];
    for (int f = 0; f < 4; ++f) {
        d_idx[f] = lists.dev<int32_t>(idx[f]);
        d_off[f] = lists.dev<uint64_t>(off[f]);
    }
    unsigned long long *m2r = (unsigned long long *)(pw + g.off_m2r), *m2c = (unsigned long long *)(pw + g.off_m2c);
    unsigned long long *m1r = (unsigned long long *)(pw + g.off_m1r), *m1c = (unsigned long long *)(pw + g.off_m1c);
    int rc = launch_masks(ctx, d_idx[2], d_off[2], row_off2, 0, (uint32_t)n2, g.stride_r, m2r, stream);
    if (rc != PGX_OK) return rc;
    rc = launch_masks(ctx, d_idx[3], d_off[3], col_off2, 0, (uint32_t)n2, g.stride_c, m2c, stream);
    if (rc != PGX_OK) return rc;
    rc = match_blocks(ctx, (uint32_t)n1, (uint32_t)n2, g, m2r, m2c, res.dev<long long>(r_match),
                      res.dev<unsigned long long>(r_overlap), res.dev<unsigned long long>(r_total),
                      (unsigned long long *)mat.dev_if(out_matrix, r_matrix), (unsigned long long *)(pw + g.off_o),
                      (uint8_t *)(pw + g.off_flags), stream,
                      [&](uint32_t b0, uint32_t nb, const unsigned long long **a, const unsigned long long **b) {
                          int r = launch_masks(ctx, d_idx[0], d_off[0], row_off1, b0, nb, g.stride_r, m1r, stream);
                          if (r == PGX_OK) r = launch_masks(ctx, d_idx[1], d_off[1], col_off1, b0, nb, g.stride_c, m1c, stream);
                          *a = m1r;
                          *b = m1c;
                          return r;
                      });
    if (rc != PGX_OK) return rc;
    PGX_HIP(res.download(stream));
    PGX_HIP(mat.download(stream));
    PGX_HIP(hipStreamSynchronize(stream));
    return PGX_OK;
}

}  // namespace

extern "C" {

size_t pgx_fcd_match_workspace_bytes(uint32_t n_rows, uint32_t n_cols, uint64_t n1, uint64_t n2) {
    if (match_sizes_bad(n_rows, n_cols, n1, n2)) return 0;
    return match_geom(n_rows, n_cols, n2).bytes;
}

int pgx_fcd_match(pgx_ctx *ctx, uint32_t n_rows, uint32_t n_cols, const int32_t *rows1, const uint64_t *row_off1,
                  const int32_t *cols1, const uint64_t *col_off1, uint64_t n1, const int32_t *rows2, const uint64_t *row_off2,
                  const int32_t *cols2, const uint64_t *col_off2, uint64_t n2, int64_t *out_match, uint64_t *out_overlap,
                  uint64_t *out_total, uint64_t *out_matrix) {
    return guarded(__func__, [&] {
        return match_host(ctx, n_rows, n_cols, rows1, row_off1, cols1, col_off1, n1, rows2, row_off2, cols2, col_off2, n2,
                          out_match, out_overlap, out_total, out_matrix);
    });
}

int pgx_fcd_match_dev(pgx_ctx *ctx, const uint64_t *d_row_masks1, const uint64_t *d_col_masks1, uint64_t n1,
                      const uint64_t *d_row_masks2, const uint64_t *d_col_masks2, uint64_t n2, uint32_t n_rows,
                      uint32_t n_cols, int64_t *d_match, uint64_t *d_overlap, uint64_t *d_total, uint64_t *d_matrix,
                      void *d_workspace, size_t workspace_bytes, void *stream) {
    return guarded(__func__, [&] {
        return match_dev(ctx, d_row_masks1, d_col_masks1, n1, d_row_masks2, d_col_masks2, n2, n_rows, n_cols, d_match,
                         d_overlap, d_total, d_matrix, d_workspace, workspace_bytes, (hipStream_t)stream);
    });
}

}  // extern "C"
