// Formal concept decomposition of a binary table on the genome-major bitmap (reference fcd.py,
// formal_concept_decomposition / compute_concept_coverage; Algorithm 2 of doi:10.1016/j.jcss.2009.05.002).
//
// The table is covered greedily with all-ones blocks ("concepts": a set of rows x a set of genomes). A concept grows one
// genome column at a time; every step of that growth is "for each live column, count the ones among the rows still in
// play", i.e. a masked popcount  cnt[c] = popcount(U[:, c] & acc)  over the bitmap of the uncovered ones U and the row
// mask acc. The reference forms that count by copying a dense int64 block with np.ix_ and summing it.
//
// State on the device (pgx_fcd_workspace_bytes): U (a working copy of the table, the caller's bitmap is never written),
// acc (stride words), w (overlap only: ones of U per row among the merged columns), raw scores, live flags, the ones left
// per column, the merged columns, the row list of the finished concept and a 32-byte result record.
//
// Per step: fcd_score_kernel (one workgroup per live column and 16 KB chunk of it, 16-byte loads, lanes whose acc words
// are all zero do not touch the column), fcd_select_kernel (one workgroup: scores from the raw counts, arg max with the
// lowest index among ties, raw counts zeroed for the next step), 16 bytes back to the host, which makes the `>` test and
// launches fcd_merge_kernel (acc &= column). Per concept: fcd_begin_kernel (acc = rows with a one left, live = columns
// with a one left), fcd_compact_kernel (acc's set bits -> ascending row indices), fcd_clear_kernel (clear the block in U,
// count what it cleared). Plain launches on one stream; the host loops are bounded by n_genomes steps per concept and
// `limit` concepts. No workgroup waits for another.
#include <vector>

#include "pgx_internal.h"

namespace {

constexpr int FC_THREADS = 256;
constexpr uint32_t FC_CHUNK = 1024;   // 16-byte lanes of a column per workgroup of the score / clear kernels (16 KB)

struct FcdResult {          // device record read back by the host
    int32_t idx;            // fcd_select_kernel: best live column, -1 = none live
    int32_t pad;
    uint64_t score;         // its score: int64, or the bits of a double (dim_balance)
    uint64_t n_rows;        // fcd_compact_kernel: rows of the concept
    uint64_t cleared;       // fcd_clear_kernel: ones the concept cleared
};
static_assert(sizeof(FcdResult) == 32, "read back as 16 or 32 bytes");

struct FcdGeom {
    uint32_t stride, lanes, chunks;
    size_t off_u, off_acc, off_w, off_raw, off_live, off_colcnt, off_cols, off_rows, off_res, bytes;
};

FcdGeom make_geom(uint32_t n_rows, uint32_t n_genomes) {
    FcdGeom g;
    g.stride = pgx_bitmap_stride_words(n_rows);
    g.lanes = g.stride / 2;                              // (stride is a multiple of 16 words)
    g.chunks = ceil_div_u32(g.lanes, FC_CHUNK);
    WsLayout ws;
    g.off_u = ws.take((size_t)n_genomes * g.stride * 8);
    g.off_acc = ws.take((size_t)g.stride * 8);
    g.off_w = ws.take((size_t)g.stride * 64 * 4);        // one counter per bit of a column, pad bits included
    g.off_raw = ws.take((size_t)n_genomes * 8);
    g.off_live = ws.take((size_t)n_genomes * 4);
    g.off_colcnt = ws.take((size_t)n_genomes * 8);
    g.off_cols = ws.take((size_t)n_genomes * 4);
    g.off_rows = ws.take((size_t)n_rows * 4);
    g.off_res = ws.take(sizeof(FcdResult));
    g.bytes = ws.off;
    return g;
}

__device__ __forceinline__ uint32_t popc128(const uint4 &v) {
    return __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
}

__device__ __forceinline__ uint4 and128(const uint4 &a, const uint4 &b) {
    return make_uint4(a.x & b.x, a.y & b.y, a.z & b.z, a.w & b.w);
}

// sum over the workgroup's waves into *dst (integers: the order of the additions does not matter)
__device__ __forceinline__ void wave_add(unsigned long long sum, unsigned long long *dst) {
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
    if ((threadIdx.x & 63u) == 0 && sum) atomicAdd(dst, sum);
}

// raw[c] += popcount(U[:, c] & acc) over this workgroup's chunk of column c; OVERLAP: + the sum of w[r] over the set
// bits of S[:, c] & acc. Columns that are not live are left alone (raw stays 0).
template <bool OVERLAP>
__global__ __launch_bounds__(FC_THREADS) void fcd_score_kernel(const uint4 *__restrict__ U, const uint4 *__restrict__ S,
                                                               const uint4 *__restrict__ acc, const uint32_t *__restrict__ w,
                                                               const uint32_t *__restrict__ live, uint32_t lanes,
                                                               unsigned long long *__restrict__ raw) {
    const uint32_t c = blockIdx.x;
    if (!live[c]) return;                                 // (uniform over the workgroup)
    const uint32_t l0 = blockIdx.y * FC_CHUNK;
    const uint32_t l1 = min(l0 + FC_CHUNK, lanes);
    const size_t col = (size_t)c * lanes;
    unsigned long long sum = 0;
    for (uint32_t l = l0 + threadIdx.x; l < l1; l += FC_THREADS) {
        const uint4 a = acc[l];
        if ((a.x | a.y | a.z | a.w) == 0u) continue;      // no row of these 128 is in play: the column is not read
        sum += popc128(and128(U[col + l], a));
        if (OVERLAP) {
            const uint4 s = and128(S[col + l], a);
            const uint32_t m[4] = {s.x, s.y, s.z, s.w};   // bit b of m[k] = row 128 l + 32 k + b
#pragma unroll
            for (int k = 0; k < 4; ++k)
                for (uint32_t mm = m[k]; mm; mm &= mm - 1u) sum += w[(size_t)l * 128u + k * 32u + (__ffs(mm) - 1)];
        }
    }
    wave_add(sum, &raw[c]);
}

// is score a (column ia) to be preferred to score b (column ib)? np.argmax's rule: the largest, the first among equals,
// and a nan counts as the largest.
__device__ __forceinline__ bool better_i(long long a, int ia, long long b, int ib) {
    if (ib < 0) return ia >= 0;
    if (ia < 0) return false;
    return a > b || (a == b && ia < ib);
}
__device__ __forceinline__ bool better_d(double a, int ia, double b, int ib) {
    if (ib < 0) return ia >= 0;
    if (ia < 0) return false;
    const bool na = a != a, nb = b != b;
    if (na || nb) return na && (!nb || ia < ib);
    return a > b || (a == b && ia < ib);
}

// One workgroup. score[c] = mult * raw[c] (int64), or factor * (double)raw[c] (USE_F64: ONE float64 multiply, the factor
// comes from the host) for every live column; the best one and its score go to res; raw is zeroed for the next step.
template <bool USE_F64>
__global__ __launch_bounds__(FC_THREADS) void fcd_select_kernel(unsigned long long *__restrict__ raw,
                                                                const uint32_t *__restrict__ live, uint32_t S,
                                                                long long mult, double factor, FcdResult *__restrict__ res) {
    __shared__ long long s_i[FC_THREADS];
    __shared__ double s_d[FC_THREADS];
    __shared__ int s_idx[FC_THREADS];
    long long bi = 0;
    double bd = 0.0;
    int bidx = -1;
    for (uint32_t c = threadIdx.x; c < S; c += FC_THREADS) {   // ascending: a thread keeps its first maximum
        if (!live[c]) continue;
        const unsigned long long v = raw[c];
        raw[c] = 0ull;
        if (USE_F64) {
            const double x = factor * (double)v;
            if (better_d(x, (int)c, bd, bidx)) { bd = x; bidx = (int)c; }
        } else {
            const long long x = mult * (long long)v;
            if (better_i(x, (int)c, bi, bidx)) { bi = x; bidx = (int)c; }
        }
    }
    s_i[threadIdx.x] = bi; s_d[threadIdx.x] = bd; s_idx[threadIdx.x] = bidx;
    __syncthreads();
    for (uint32_t d = FC_THREADS / 2; d > 0; d >>= 1) {
        if (threadIdx.x < d) {
            const uint32_t o = threadIdx.x + d;
            const bool take = USE_F64 ? better_d(s_d[o], s_idx[o], s_d[threadIdx.x], s_idx[threadIdx.x])
                                      : better_i(s_i[o], s_idx[o], s_i[threadIdx.x], s_idx[threadIdx.x]);
            if (take) { s_i[threadIdx.x] = s_i[o]; s_d[threadIdx.x] = s_d[o]; s_idx[threadIdx.x] = s_idx[o]; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        res->idx = s_idx[0];
        res->score = USE_F64 ? (uint64_t)__double_as_longlong(s_d[0]) : (uint64_t)s_i[0];
    }
}

// a concept's start: acc = the rows with a one left in U, live = the columns with a one left (colcnt)
__global__ __launch_bounds__(FC_THREADS) void fcd_begin_kernel(const unsigned long long *__restrict__ U, uint32_t stride,
                                                               uint32_t S, const unsigned long long *__restrict__ colcnt,
                                                               unsigned long long *__restrict__ acc,
                                                               uint32_t *__restrict__ live) {
    const uint32_t i = blockIdx.x * FC_THREADS + threadIdx.x;
    if (i < stride) {
        unsigned long long any = 0;
        for (uint32_t c = 0; c < S; ++c) any |= U[(size_t)c * stride + i];
        acc[i] = any;
    }
    if (i < S) live[i] = colcnt[i] != 0ull;
}

// column c joins the concept as its k-th: acc &= src[:, c] (src = U, or the table itself under overlap)
__global__ __launch_bounds__(FC_THREADS) void fcd_merge_kernel(const unsigned long long *__restrict__ src_col, uint32_t stride,
                                                               unsigned long long *__restrict__ acc,
                                                               uint32_t *__restrict__ live, int32_t *__restrict__ cols,
                                                               uint32_t c, uint32_t k) {
    const uint32_t i = blockIdx.x * FC_THREADS + threadIdx.x;
    if (i < stride) acc[i] &= src_col[i];
    if (i == 0) { live[c] = 0u; cols[k] = (int32_t)c; }
}

// overlap: w[r] += U[r, c] for the column that has just joined
__global__ __launch_bounds__(FC_THREADS) void fcd_w_add_kernel(const unsigned long long *__restrict__ u_col, uint32_t n_bits,
                                                               uint32_t *__restrict__ w) {
    const uint32_t r = blockIdx.x * FC_THREADS + threadIdx.x;
    if (r < n_bits) w[r] += (uint32_t)((u_col[r >> 6] >> (r & 63u)) & 1ull);
}

// colcnt[c] = ones of column c
__global__ __launch_bounds__(FC_THREADS) void fcd_col_count_kernel(const uint4 *__restrict__ U, uint32_t lanes,
                                                                   unsigned long long *__restrict__ colcnt) {
    __shared__ unsigned long long total;
    if (threadIdx.x == 0) total = 0ull;
    __syncthreads();
    unsigned long long sum = 0;
    for (uint32_t l = threadIdx.x; l < lanes; l += FC_THREADS) sum += popc128(U[(size_t)blockIdx.x * lanes + l]);
    wave_add(sum, &total);
    __syncthreads();
    if (threadIdx.x == 0) colcnt[blockIdx.x] = total;
}

// One workgroup: the set bits of acc as ascending row indices; res->n_rows = how many; res->cleared = 0 for the clear
// kernel that follows. 1024 words per round: popcounts, an inclusive scan in LDS, every thread writes its word's rows.
__global__ __launch_bounds__(1024) void fcd_compact_kernel(const unsigned long long *__restrict__ acc, uint32_t words,
                                                           uint32_t n_rows, int32_t *__restrict__ rows_out,
                                                           FcdResult *__restrict__ res) {
    __shared__ uint32_t scan[1024];
    __shared__ uint32_t base;
    if (threadIdx.x == 0) base = 0u;
    __syncthreads();
    for (uint32_t w0 = 0; w0 < words; w0 += 1024u) {
        const uint32_t wi = w0 + threadIdx.x;
        unsigned long long word = wi < words ? acc[wi] : 0ull;
        const uint32_t n = (uint32_t)__popcll(word);
        scan[threadIdx.x] = n;
        __syncthreads();
        for (uint32_t d = 1; d < 1024u; d <<= 1) {
            const uint32_t t = threadIdx.x >= d ? scan[threadIdx.x - d] : 0u;
            __syncthreads();
            scan[threadIdx.x] += t;
            __syncthreads();
        }
        uint32_t off = base + scan[threadIdx.x] - n;
        for (; word; word &= word - 1ull, ++off)          // (rows_out holds n_rows entries: a set pad bit writes nothing)
            if (off < n_rows) rows_out[off] = (int32_t)(wi * 64u + (uint32_t)(__ffsll((long long)word) - 1));
        __syncthreads();
        if (threadIdx.x == 1023u) base += scan[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) { res->n_rows = base; res->cleared = 0ull; }
}

// Clear the block (rows of mask) x (columns cols[0..gridDim.x)) in U: *cleared += the ones it held, colcnt follows.
// A column must not be listed twice.
__global__ __launch_bounds__(FC_THREADS) void fcd_clear_kernel(uint4 *__restrict__ U, const uint4 *__restrict__ mask,
                                                               const int32_t *__restrict__ cols, uint32_t lanes,
                                                               unsigned long long *__restrict__ colcnt,
                                                               unsigned long long *__restrict__ cleared) {
    const uint32_t c = (uint32_t)cols[blockIdx.x];
    const uint32_t l0 = blockIdx.y * FC_CHUNK;
    const uint32_t l1 = min(l0 + FC_CHUNK, lanes);
    const size_t col = (size_t)c * lanes;
    __shared__ unsigned long long total;
    if (threadIdx.x == 0) total = 0ull;
    __syncthreads();
    unsigned long long sum = 0;
    for (uint32_t l = l0 + threadIdx.x; l < l1; l += FC_THREADS) {
        const uint4 a = mask[l];
        if ((a.x | a.y | a.z | a.w) == 0u) continue;
        const uint4 u = U[col + l];
        sum += popc128(and128(u, a));
        U[col + l] = make_uint4(u.x & ~a.x, u.y & ~a.y, u.z & ~a.z, u.w & ~a.w);
    }
    wave_add(sum, &total);
    __syncthreads();
    if (threadIdx.x == 0 && total) {
        atomicAdd(&colcnt[c], 0ull - total);
        atomicAdd(cleared, total);
    }
}

// mask |= the bits of rows[0..n) (coverage: a concept's rows as a mask; rows are checked on the host)
__global__ __launch_bounds__(FC_THREADS) void fcd_rows_to_mask_kernel(const int32_t *__restrict__ rows, uint64_t n,
                                                                      unsigned long long *__restrict__ mask) {
    const uint64_t k = (uint64_t)blockIdx.x * FC_THREADS + threadIdx.x;
    if (k < n) {
        const uint32_t r = (uint32_t)rows[k];
        atomicOr(&mask[r >> 6], 1ull << (r & 63u));
    }
}

struct FcdWs {
    FcdGeom g;
    unsigned long long *U, *acc, *raw, *colcnt;
    uint32_t *w, *live;
    int32_t *cols, *rows;
    FcdResult *res;
    FcdWs(void *d_ws, uint32_t n_rows, uint32_t n_genomes) : g(make_geom(n_rows, n_genomes)) {
        char *p = (char *)d_ws;
        U = (unsigned long long *)(p + g.off_u); acc = (unsigned long long *)(p + g.off_acc);
        w = (uint32_t *)(p + g.off_w); raw = (unsigned long long *)(p + g.off_raw);
        live = (uint32_t *)(p + g.off_live); colcnt = (unsigned long long *)(p + g.off_colcnt);
        cols = (int32_t *)(p + g.off_cols); rows = (int32_t *)(p + g.off_rows); res = (FcdResult *)(p + g.off_res);
    }
};

// U = a copy of d_bits, colcnt = its ones per column, raw = 0; *ones = the ones of the table (stream synchronised)
int fcd_prepare(pgx_ctx *ctx, const FcdWs &ws, const uint64_t *d_bits, uint32_t S, hipStream_t stream, uint64_t *ones) {
    const size_t nbits = (size_t)S * ws.g.stride * 8;
    PGX_HIP(hipMemcpyAsync(ws.U, d_bits, nbits, hipMemcpyDeviceToDevice, stream));
    PGX_HIP(hipMemsetAsync(ws.raw, 0, (size_t)S * 8, stream));
    {
        ProfScope prof(ctx, "fcd_col_count_kernel", stream);
        fcd_col_count_kernel<<<S, FC_THREADS, 0, stream>>>((const uint4 *)ws.U, ws.g.lanes, ws.colcnt);
    }
    PGX_HIP(hipGetLastError());
    std::vector<uint64_t> cnt(S);
    PGX_HIP(hipMemcpyAsync(cnt.data(), ws.colcnt, (size_t)S * 8, hipMemcpyDeviceToHost, stream));
    PGX_HIP(hipStreamSynchronize(stream));
    *ones = 0;
    for (uint64_t c : cnt) *ones += c;
    return PGX_OK;
}

void fcd_reset_result(pgx_ctx *ctx) {
    ctx->fcd_rows.clear(); ctx->fcd_cols.clear(); ctx->fcd_left.clear();
    ctx->fcd_row_off.assign(1, 0); ctx->fcd_col_off.assign(1, 0);
}

// The decomposition of the table in d_bits (device, never written); the concepts are kept in the context for pgx_fcd_fetch.
int fcd_run(pgx_ctx *ctx, const uint64_t *d_bits, uint32_t n_rows, uint32_t S, uint64_t limit, uint32_t flags,
            const double *dim_factors, void *d_ws, size_t ws_bytes, hipStream_t stream, pgx_fcd_info_t *info) {
    PGX_REQUIRE(ctx && info, "NULL argument");
    memset(info, 0, sizeof(*info));
    fcd_reset_result(ctx);
    PGX_REQUIRE((flags & ~(uint32_t)(PGX_FCD_OVERLAP | PGX_FCD_DIM_BALANCE)) == 0, "unknown flag");
    PGX_REQUIRE((uint64_t)n_rows < (1ull << 31) && S < (1u << 31), "table too large");
    if (n_rows == 0 || S == 0) return PGX_OK;
    PGX_REQUIRE(d_bits && d_ws, "NULL argument");
    PGX_REQUIRE((((uintptr_t)d_bits | (uintptr_t)d_ws) & 15u) == 0, "bitmap and workspace must be 16-byte aligned");
    const bool overlap = (flags & PGX_FCD_OVERLAP) != 0;
    const bool f64 = !overlap && (flags & PGX_FCD_DIM_BALANCE) != 0;
    PGX_REQUIRE(!f64 || dim_factors, "dim_balance needs the factor of every step");
    const FcdWs ws(d_ws, n_rows, S);
    PGX_REQUIRE(ws_bytes >= ws.g.bytes, "workspace too small (see pgx_fcd_workspace_bytes)");
    HostVec<FcdResult> h_res(ctx, FC_HOST_RES, 1);
    if (!h_res.ok()) { pgx_set_error("%s: out of page-locked host memory", __func__); return PGX_ERR_NOMEM; }

    uint64_t left = 0;
    int rc = fcd_prepare(ctx, ws, d_bits, S, stream, &left);
    if (rc != PGX_OK) return rc;
    info->ones_total = left;
    const uint32_t stride = ws.g.stride, lanes = ws.g.lanes;
    const uint32_t word_blocks = ceil_div_u32(std::max(stride, S), FC_THREADS);
    const dim3 col_grid(S, ws.g.chunks);
    const uint4 *S4 = (const uint4 *)d_bits;
    uint64_t n_concepts = 0;
    while (left > 0 && n_concepts < limit) {
        if (overlap) PGX_HIP(hipMemsetAsync(ws.w, 0, (size_t)stride * 64 * 4, stream));
        {
            ProfScope prof(ctx, "fcd_begin_kernel", stream);
            fcd_begin_kernel<<<word_blocks, FC_THREADS, 0, stream>>>(ws.U, stride, S, ws.colcnt, ws.acc, ws.live);
        }
        PGX_HIP(hipGetLastError());
        uint32_t k = 0;                       // columns merged so far (at most S: every merge takes one out of live)
        long long cur_i = 0;
        double cur_d = 0.0;
        while (k < S) {
            {
                ProfScope prof(ctx, "fcd_score_kernel", stream);
                if (overlap)
                    fcd_score_kernel<true><<<col_grid, FC_THREADS, 0, stream>>>((const uint4 *)ws.U, S4, (const uint4 *)ws.acc,
                                                                                 ws.w, ws.live, lanes, ws.raw);
                else
                    fcd_score_kernel<false><<<col_grid, FC_THREADS, 0, stream>>>((const uint4 *)ws.U, S4, (const uint4 *)ws.acc,
                                                                                  ws.w, ws.live, lanes, ws.raw);
            }
            PGX_HIP(hipGetLastError());
            {
                ProfScope prof(ctx, "fcd_select_kernel", stream);
                if (f64) fcd_select_kernel<true><<<1, FC_THREADS, 0, stream>>>(ws.raw, ws.live, S, 0, dim_factors[k], ws.res);
                else fcd_select_kernel<false><<<1, FC_THREADS, 0, stream>>>(ws.raw, ws.live, S, overlap ? 1 : (long long)k + 1,
                                                                             0.0, ws.res);
            }
            PGX_HIP(hipGetLastError());
            PGX_HIP(hipMemcpyAsync(h_res.data(), ws.res, 16, hipMemcpyDeviceToHost, stream));
            PGX_HIP(hipStreamSynchronize(stream));
            ++info->steps;
            const int32_t c = h_res[0].idx;
            if (c < 0) break;                                         // no live column left
            PGX_REQUIRE((uint32_t)c < S, "column out of range");
            double score_d;
            memcpy(&score_d, &h_res[0].score, 8);
            const long long score_i = (long long)h_res[0].score;
            if (!(f64 ? score_d > cur_d : score_i > cur_i)) break;    // the concept does not grow any more
            cur_d = score_d; cur_i = score_i;
            {
                ProfScope prof(ctx, "fcd_merge_kernel", stream);
                fcd_merge_kernel<<<ceil_div_u32(stride, FC_THREADS), FC_THREADS, 0, stream>>>(
                    (overlap ? (const unsigned long long *)d_bits : ws.U) + (size_t)c * stride, stride, ws.acc, ws.live, ws.cols,
                    (uint32_t)c, k);
            }
            PGX_HIP(hipGetLastError());
            if (overlap) {
                ProfScope prof(ctx, "fcd_w_add_kernel", stream);
                fcd_w_add_kernel<<<ceil_div_u32(stride * 64u, FC_THREADS), FC_THREADS, 0, stream>>>(ws.U + (size_t)c * stride,
                                                                                                   stride * 64u, ws.w);
                PGX_HIP(hipGetLastError());
            }
            ctx->fcd_cols.push_back(c);
            ++k;
        }
        if (k == 0) {      // ones are left but no column scores above zero: the reference would loop forever
            pgx_set_error("%s: no concept found although %llu ones are uncovered", __func__, (unsigned long long)left);
            return PGX_ERR_INTERNAL;
        }
        {
            ProfScope prof(ctx, "fcd_compact_kernel", stream);
            fcd_compact_kernel<<<1, 1024, 0, stream>>>(ws.acc, stride, n_rows, ws.rows, ws.res);
        }
        PGX_HIP(hipGetLastError());
        {
            ProfScope prof(ctx, "fcd_clear_kernel", stream);
            fcd_clear_kernel<<<dim3(k, ws.g.chunks), FC_THREADS, 0, stream>>>((uint4 *)ws.U, (const uint4 *)ws.acc, ws.cols, lanes,
                                                                              ws.colcnt, (unsigned long long *)&ws.res->cleared);
        }
        PGX_HIP(hipGetLastError());
        PGX_HIP(hipMemcpyAsync(h_res.data(), ws.res, 32, hipMemcpyDeviceToHost, stream));
        PGX_HIP(hipStreamSynchronize(stream));
        const uint64_t n = h_res[0].n_rows, cleared = h_res[0].cleared;
        PGX_REQUIRE(n <= n_rows && cleared <= left, "inconsistent concept");
        if (cleared == 0) {   // the reference would find the same concept again, for ever
            pgx_set_error("%s: a concept cleared nothing", __func__);
            return PGX_ERR_INTERNAL;
        }
        const size_t at = ctx->fcd_rows.size();
        ctx->fcd_rows.resize(at + n);
        PGX_HIP(hipMemcpyAsync(ctx->fcd_rows.data() + at, ws.rows, n * 4, hipMemcpyDeviceToHost, stream));
        PGX_HIP(hipStreamSynchronize(stream));
        left -= cleared;
        ctx->fcd_row_off.push_back(ctx->fcd_rows.size());
        ctx->fcd_col_off.push_back(ctx->fcd_cols.size());
        ctx->fcd_left.push_back(left);
        ++n_concepts;
    }
    info->n_concepts = n_concepts;
    info->n_row_entries = ctx->fcd_rows.size();
    info->n_col_entries = ctx->fcd_cols.size();
    info->ones_left = left;
    return PGX_OK;
}

int fcd_host(pgx_ctx *ctx, const int32_t *rows, const int32_t *genomes, uint64_t n_records, uint32_t n_rows, uint32_t S,
             uint64_t limit, uint32_t flags, const double *dim_factors, pgx_fcd_info_t *info, uint64_t *out_duplicates) {
    PGX_REQUIRE(ctx && info, "NULL argument");
    PGX_REQUIRE(n_records == 0 || (rows && genomes), "NULL record arrays");
    PGX_HIP(hipSetDevice(ctx->device_id));
    memset(info, 0, sizeof(*info));
    fcd_reset_result(ctx);
    DevBuf d_bits(ctx, FC_SLOT_BITS), d_cnt(ctx, FC_SLOT_CNT), d_ws(ctx, FC_SLOT_WS);
    uint64_t dup = 0;
    const int rc = pgx_load_coo_bitmap(ctx, rows, genomes, n_records, n_rows, S, FC_SLOT_ROWS, FC_SLOT_GENOMES, d_bits, d_cnt, &dup);
    if (rc != PGX_OK) return rc;
    if (out_duplicates) *out_duplicates = dup;
    if (dup) return PGX_OK;                   // not a 0/1 table: nothing is decomposed
    const size_t nws = make_geom(n_rows, S).bytes;
    PGX_HIP(d_ws.alloc(nws));
    return fcd_run(ctx, d_bits.as<uint64_t>(), n_rows, S, limit, flags, dim_factors, d_ws.p, nws, ctx->stream, info);
}

int fcd_resident(pgx_ctx *ctx, uint64_t token, const int32_t *row_map, const int32_t *col_map, uint32_t G, uint32_t S,
                 uint64_t limit, uint32_t flags, const double *dim_factors, pgx_fcd_info_t *info) {
    PGX_REQUIRE(ctx && info, "NULL argument");
    PGX_REQUIRE(G == 0 || row_map, "NULL row map");
    ResidentBitmap src;
    int rc = pgx_resident_bitmap(ctx, token, S, &src);
    if (rc != PGX_OK) return rc;
    PGX_REQUIRE((uint64_t)G < (1ull << 31), "table too large");
    PGX_HIP(hipSetDevice(ctx->device_id));
    DevBuf d_map(ctx, FC_SLOT_MAP), d_cmap(ctx, FC_SLOT_CMAP), d_bits(ctx, FC_SLOT_BITS), d_ws(ctx, FC_SLOT_WS);
    rc = pgx_gather_resident(ctx, src, row_map, col_map, G, S, d_map, &d_cmap, d_bits, "fcd_gather_kernel");
    if (rc != PGX_OK) return rc;
    const size_t nws = make_geom(G, S).bytes;
    PGX_HIP(d_ws.alloc(nws));
    return fcd_run(ctx, d_bits.as<uint64_t>(), G, S, limit, flags, dim_factors, d_ws.p, nws, ctx->stream, info);
}

int fcd_fetch(pgx_ctx *ctx, int32_t *out_rows, uint64_t *out_row_offsets, int32_t *out_cols, uint64_t *out_col_offsets,
              uint64_t *out_left) {
    PGX_REQUIRE(ctx && out_row_offsets && out_col_offsets, "NULL argument");
    PGX_REQUIRE(!ctx->fcd_row_off.empty(), "no decomposition on this context (pgx_fcd*)");
    PGX_REQUIRE((out_rows || ctx->fcd_rows.empty()) && (out_cols || ctx->fcd_cols.empty()) &&
                    (out_left || ctx->fcd_left.empty()), "NULL argument");
    // (row / column entries beyond the last finished concept, left by a call that failed half way, are not copied)
    const size_t nr = (size_t)ctx->fcd_row_off.back(), nc = (size_t)ctx->fcd_col_off.back();
    if (nr) memcpy(out_rows, ctx->fcd_rows.data(), nr * 4);
    if (nc) memcpy(out_cols, ctx->fcd_cols.data(), nc * 4);
    memcpy(out_row_offsets, ctx->fcd_row_off.data(), ctx->fcd_row_off.size() * 8);
    memcpy(out_col_offsets, ctx->fcd_col_off.data(), ctx->fcd_col_off.size() * 8);
    if (!ctx->fcd_left.empty()) memcpy(out_left, ctx->fcd_left.data(), ctx->fcd_left.size() * 8);
    return PGX_OK;
}

int fcd_coverage(pgx_ctx *ctx, const int32_t *rows, const int32_t *genomes, uint64_t n_records, uint32_t n_rows, uint32_t S,
                 const int32_t *c_rows, const uint64_t *c_row_off, const int32_t *c_cols, const uint64_t *c_col_off,
                 uint64_t n_concepts, uint64_t *out_cleared, uint64_t *out_ones, uint64_t *out_duplicates) {
    PGX_REQUIRE(ctx && out_ones, "NULL argument");
    PGX_REQUIRE(n_records == 0 || (rows && genomes), "NULL record arrays");
    PGX_REQUIRE(n_concepts == 0 || (c_row_off && c_col_off && out_cleared), "NULL argument");
    PGX_REQUIRE((uint64_t)n_rows < (1ull << 31) && S < (1u << 31), "table too large");
    const uint64_t nr = n_concepts ? c_row_off[n_concepts] : 0, nc = n_concepts ? c_col_off[n_concepts] : 0;
    PGX_REQUIRE((nr == 0 || c_rows) && (nc == 0 || c_cols), "NULL argument");
    std::vector<uint64_t> seen((S + 63) / 64 + 1);
    for (uint64_t i = 0; i < n_concepts; ++i) {
        PGX_REQUIRE(c_row_off[i] <= c_row_off[i + 1] && c_col_off[i] <= c_col_off[i + 1] && c_row_off[i + 1] <= nr &&
                        c_col_off[i + 1] <= nc && c_col_off[i + 1] - c_col_off[i] <= S, "concept offsets out of order");
        for (uint64_t k = c_row_off[i]; k < c_row_off[i + 1]; ++k)
            PGX_REQUIRE(c_rows[k] >= 0 && (uint32_t)c_rows[k] < n_rows, "concept row out of range");
        std::fill(seen.begin(), seen.end(), 0);
        for (uint64_t k = c_col_off[i]; k < c_col_off[i + 1]; ++k) {
            PGX_REQUIRE(c_cols[k] >= 0 && (uint32_t)c_cols[k] < S, "concept column out of range");
            uint64_t &wd = seen[(uint32_t)c_cols[k] >> 6];
            PGX_REQUIRE(!(wd >> ((uint32_t)c_cols[k] & 63u) & 1ull), "a concept lists a column twice");
            wd |= 1ull << ((uint32_t)c_cols[k] & 63u);
        }
    }
    PGX_HIP(hipSetDevice(ctx->device_id));
    *out_ones = 0;
    DevBuf d_bits(ctx, FC_SLOT_BITS), d_cnt(ctx, FC_SLOT_CNT), d_ws(ctx, FC_SLOT_WS), d_crows(ctx, FC_SLOT_CROWS),
        d_ccols(ctx, FC_SLOT_CCOLS), d_cleared(ctx, FC_SLOT_CLEARED);
    uint64_t dup = 0;
    int rc = pgx_load_coo_bitmap(ctx, rows, genomes, n_records, n_rows, S, FC_SLOT_ROWS, FC_SLOT_GENOMES, d_bits, d_cnt, &dup);
    if (rc != PGX_OK) return rc;
    if (out_duplicates) *out_duplicates = dup;
    if (dup || n_rows == 0 || S == 0) {
        for (uint64_t i = 0; i < n_concepts; ++i) out_cleared[i] = 0;
        return PGX_OK;
    }
    const size_t nws = make_geom(n_rows, S).bytes;
    PGX_HIP(d_ws.alloc(nws));
    const FcdWs ws(d_ws.p, n_rows, S);
    hipStream_t stream = ctx->stream;
    rc = fcd_prepare(ctx, ws, d_bits.as<uint64_t>(), S, stream, out_ones);
    if (rc != PGX_OK || n_concepts == 0) return rc;
    PGX_HIP(d_crows.alloc(nr * 4));
    PGX_HIP(d_ccols.alloc(nc * 4));
    PGX_HIP(d_cleared.alloc(n_concepts * 8));
    if (nr) PGX_HIP(hipMemcpyAsync(d_crows.p, c_rows, nr * 4, hipMemcpyHostToDevice, stream));
    if (nc) PGX_HIP(hipMemcpyAsync(d_ccols.p, c_cols, nc * 4, hipMemcpyHostToDevice, stream));
    PGX_HIP(hipMemsetAsync(d_cleared.p, 0, n_concepts * 8, stream));
    for (uint64_t i = 0; i < n_concepts; ++i) {
        const uint64_t n = c_row_off[i + 1] - c_row_off[i], k = c_col_off[i + 1] - c_col_off[i];
        if (n == 0 || k == 0) continue;
        PGX_HIP(hipMemsetAsync(ws.acc, 0, (size_t)ws.g.stride * 8, stream));
        {
            ProfScope prof(ctx, "fcd_rows_to_mask_kernel", stream);
            fcd_rows_to_mask_kernel<<<(uint32_t)((n + FC_THREADS - 1) / FC_THREADS), FC_THREADS, 0, stream>>>(
                d_crows.as<int32_t>() + c_row_off[i], n, ws.acc);
        }
        PGX_HIP(hipGetLastError());
        {
            ProfScope prof(ctx, "fcd_clear_kernel", stream);
            fcd_clear_kernel<<<dim3((uint32_t)k, ws.g.chunks), FC_THREADS, 0, stream>>>(
                (uint4 *)ws.U, (const uint4 *)ws.acc, d_ccols.as<int32_t>() + c_col_off[i], ws.g.lanes, ws.colcnt,
                d_cleared.as<unsigned long long>() + i);
        }
        PGX_HIP(hipGetLastError());
    }
    PGX_HIP(hipMemcpyAsync(out_cleared, d_cleared.p, n_concepts * 8, hipMemcpyDeviceToHost, stream));
    PGX_HIP(hipStreamSynchronize(stream));
    return PGX_OK;
}

}  // namespace

extern "C" {

size_t pgx_fcd_workspace_bytes(uint32_t n_rows, uint32_t n_genomes) {
    return make_geom(n_rows, n_genomes).bytes;
}

int pgx_fcd_dev(pgx_ctx *ctx, const uint64_t *d_bits, uint32_t n_rows, uint32_t n_genomes, uint64_t limit, uint32_t flags,
                const double *dim_factors, void *d_workspace, size_t workspace_bytes, void *stream, pgx_fcd_info_t *out_info) {
    return guarded(__func__, [&] {
        return fcd_run(ctx, d_bits, n_rows, n_genomes, limit, flags, dim_factors, d_workspace, workspace_bytes,
                       (hipStream_t)stream, out_info);
    });
}

int pgx_fcd(pgx_ctx *ctx, const int32_t *rows, const int32_t *genomes, uint64_t n_records, uint32_t n_rows,
            uint32_t n_genomes, uint64_t limit, uint32_t flags, const double *dim_factors, pgx_fcd_info_t *out_info,
            uint64_t *out_duplicates) {
    return guarded(__func__, [&] {
        return fcd_host(ctx, rows, genomes, n_records, n_rows, n_genomes, limit, flags, dim_factors, out_info, out_duplicates);
    });
}

int pgx_fcd_resident(pgx_ctx *ctx, uint64_t token, const int32_t *row_map, const int32_t *col_map, uint32_t n_rows,
                     uint32_t n_genomes, uint64_t limit, uint32_t flags, const double *dim_factors, pgx_fcd_info_t *out_info) {
    return guarded(__func__, [&] {
        return fcd_resident(ctx, token, row_map, col_map, n_rows, n_genomes, limit, flags, dim_factors, out_info);
    });
}

int pgx_fcd_fetch(pgx_ctx *ctx, int32_t *out_rows, uint64_t *out_row_offsets, int32_t *out_cols, uint64_t *out_col_offsets,
                  uint64_t *out_left) {
    return guarded(__func__, [&] { return fcd_fetch(ctx, out_rows, out_row_offsets, out_cols, out_col_offsets, out_left); });
}

int pgx_fcd_coverage(pgx_ctx *ctx, const int32_t *rows, const int32_t *genomes, uint64_t n_records, uint32_t n_rows,
                     uint32_t n_genomes, const int32_t *concept_rows, const uint64_t *row_offsets, const int32_t *concept_cols,
                     const uint64_t *col_offsets, uint64_t n_concepts, uint64_t *out_cleared, uint64_t *out_ones,
                     uint64_t *out_duplicates) {
    return guarded(__func__, [&] {
        return fcd_coverage(ctx, rows, genomes, n_records, n_rows, n_genomes, concept_rows, row_offsets, concept_cols,
                            col_offsets, n_concepts, out_cleared, out_ones, out_duplicates);
    });
}

}  // extern "C"
