// Bernoulli grid likelihood of a binary gene x genome table on gfx950 (compute_bernoulli_grid_core_genome).
//
// Model: gene i occurs in genome j with probability p_i q_j. For the table X (the presence bitmap, pgx.h layout)
//   LL      = sum_ij  X_ij log(p_i q_j) + (1 - X_ij) log(1 - p_i q_j)
//   dL/dp_i = rowsum_i / p_i - sum_j (1 - X_ij) q_j / (1 - p_i q_j)
//   dL/dq_j = colsum_j / q_j - sum_i (1 - X_ij) p_i / (1 - p_i q_j)
// The optimizer (scipy's L-BFGS-B) stays on the host; one call here is one evaluation of LL and the full gradient.
//
// Every cell is evaluated with the per-cell expression the model's definition gives, term by term in fp64:
//   X = 1:  log(r) + 0 * log(1 - r)   and  0 / (1 - r)  in both gradient sums
//   X = 0:  0 * log(r) + log(1 - r)   and  q / (1 - r), p / (1 - r)
// with r = p q rounded once and 1 - r rounded once (no contraction into an fma), so that nan and inf appear where the
// per-cell expressions put them (r = 1 on a present cell: 0 * log 0 = nan, 0 / 0 = nan).
//
// Fast mode: when every r is a normal number below 1 -- decided on the device from min / max of P and Q, see
// bern_mode_kernel -- a present cell contributes exactly 0 to both gradient sums and log(p q) to LL. Its LL term is
// then taken as rowsum_i log p_i + colsum_j log q_j (one log per row and column instead of one per present cell) and
// present cells cost nothing. Absent cells cost one log and one division per pass either way.
//
// Work split (deterministic: no atomics, every partial is summed in a fixed order set by the shape alone):
//   pass A (bern_rows_kernel)  one lane per gene, blockIdx.y = a slab of genomes: the lane walks its slab's genomes
//                              (one bitmap word and one q per step, the same address across the wave) and keeps its
//                              gene's gradient sum, LL sum and present count in registers -> per-slab partials
//   pass B (bern_cols_kernel)  one lane per genome, blockIdx.y = a slab of bitmap words: the lane walks the genes of
//                              its slab (p_i the same address across the wave) -> per-slab partials of dL/dq and colsum
//   fold   (bern_fold_kernel)  one thread per gene / genome: partials summed in slab order, gradient written, the row's
//                              or column's LL term kept
//   total  (bern_total_kernel) one block: LL = the row and column terms summed in a fixed tree
// Pass B recomputes 1 - p q and a division per absent cell instead of reducing dL/dq across the lanes of pass A:
// the cross-lane sum per genome would cost about as much as the division and needs LDS or shuffles per cell.
#include <new>

#include "pgx_internal.h"

namespace {

constexpr uint32_t BN_THREADS = 256;
constexpr uint32_t BN_TARGET_WAVES = 4096;   // 256 CUs x 4 SIMDs x 4 waves
constexpr uint32_t BN_MIN_SPAN = 16;         // genomes per slab of pass A, at least

struct BernGeom {
    uint32_t stride, words;                  // bitmap words per genome; words that hold genes
    uint32_t a_slabs, a_span;                // pass A: genome slabs and genomes per slab
    uint32_t b_slabs, b_span;                // pass B: word slabs and words per slab
    size_t off_dp, off_ll, off_cnt_a, off_dq, off_cnt_b, off_terms, bytes;   // workspace layout
};

BernGeom make_geom(uint32_t G, uint32_t S) {
    BernGeom g;
    g.stride = pgx_bitmap_stride_words(G);
    g.words = (G + 63) / 64;
    const uint32_t waves_a = ceil_div_u32(G ? G : 1, 64);
    uint32_t slabs = ceil_div_u32(BN_TARGET_WAVES, waves_a);
    slabs = std::min(slabs, std::max(1u, ceil_div_u32(S, BN_MIN_SPAN)));
    g.a_span = std::max(1u, ceil_div_u32(S, slabs));
    g.a_slabs = std::max(1u, ceil_div_u32(S, g.a_span));
    const uint32_t waves_b = ceil_div_u32(S ? S : 1, 64);
    slabs = std::min(ceil_div_u32(BN_TARGET_WAVES, waves_b), std::max(1u, g.words));
    g.b_span = std::max(1u, ceil_div_u32(g.words, slabs));
    g.b_slabs = std::max(1u, ceil_div_u32(g.words, g.b_span));
    WsLayout ws;
    ws.take(256);                                            // [0, 256): the mode word
    g.off_dp = ws.take((size_t)g.a_slabs * G * 8);
    g.off_ll = ws.take((size_t)g.a_slabs * G * 8);
    g.off_cnt_a = ws.take((size_t)g.a_slabs * G * 4);
    g.off_dq = ws.take((size_t)g.b_slabs * S * 8);
    g.off_cnt_b = ws.take((size_t)g.b_slabs * S * 4);
    g.off_terms = ws.take(((size_t)G + S) * 8);
    g.bytes = ws.off;
    return g;
}

// mode[0] = 0: fast mode (every fl(p_i q_j) normal and below 1); 1: per-cell expressions everywhere. One block.
__global__ __launch_bounds__(1024) void bern_mode_kernel(const double *__restrict__ pq, uint32_t G, uint32_t S,
                                                         uint32_t force_exact, uint32_t *__restrict__ mode) {
    __shared__ double s_lo[2][1024], s_hi[2][1024];
    __shared__ int s_bad[1024];
    double lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
    int bad = 0;
    for (uint32_t k = threadIdx.x; k < G + S; k += 1024) {
        const double v = pq[k];
        const int h = k < G ? 0 : 1;
        if (!isfinite(v)) bad = 1;
        lo[h] = fmin(lo[h], v);
        hi[h] = fmax(hi[h], v);
    }
    s_lo[0][threadIdx.x] = lo[0]; s_lo[1][threadIdx.x] = lo[1];
    s_hi[0][threadIdx.x] = hi[0]; s_hi[1][threadIdx.x] = hi[1];
    s_bad[threadIdx.x] = bad;
    __syncthreads();
    for (uint32_t d = 512; d > 0; d >>= 1) {
        if (threadIdx.x < d) {
            for (int h = 0; h < 2; ++h) {
                s_lo[h][threadIdx.x] = fmin(s_lo[h][threadIdx.x], s_lo[h][threadIdx.x + d]);
                s_hi[h][threadIdx.x] = fmax(s_hi[h][threadIdx.x], s_hi[h][threadIdx.x + d]);
            }
            s_bad[threadIdx.x] |= s_bad[threadIdx.x + d];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
#pragma clang fp contract(off)
        const double pmin = s_lo[0][0], qmin = s_lo[1][0], pmax = s_hi[0][0], qmax = s_hi[1][0];
        // rounding is monotonic: for positive operands fl(pmin qmin) <= fl(p q) <= fl(pmax qmax). A subnormal
        // fl(p q) has lost bits that log p + log q keeps (fl(1e-161 * 1e-161): 0.012 in its log), so the per-cell
        // expressions take over below the smallest normal number, not only at 0.
        const bool inside = !s_bad[0] && pmin > 0.0 && qmin > 0.0 && pmin * qmin >= 0x1p-1022 && pmax * qmax < 1.0;
        mode[0] = (force_exact || !inside) ? 1u : 0u;
    }
}

__global__ __launch_bounds__(BN_THREADS) void bern_rows_kernel(const unsigned long long *__restrict__ bits,
                                                               uint32_t stride, uint32_t G, uint32_t S,
                                                               const double *__restrict__ pq, uint32_t span,
                                                               const uint32_t *__restrict__ mode,
                                                               double *__restrict__ dp_part, double *__restrict__ ll_part,
                                                               uint32_t *__restrict__ cnt_part) {
#pragma clang fp contract(off)
    const uint32_t i = blockIdx.x * BN_THREADS + threadIdx.x;
    if (i >= G) return;
    const uint32_t slab = blockIdx.y;
    const uint32_t j0 = slab * span, j1 = min(S, j0 + span);
    const bool exact = mode[0] != 0;
    const double p = pq[i];
    const double *q = pq + G;
    const uint32_t w = i >> 6, b = i & 63u;
    double g = 0.0, ll = 0.0;
    uint32_t cnt = 0;
    for (uint32_t j = j0; j < j1; ++j) {
        const unsigned long long word = bits[(size_t)j * stride + w];
        const double qj = q[j];
        if ((word >> b) & 1ull) {
            ++cnt;
            if (exact) {
                const double r = p * qj;
                const double t = 1.0 - r;
                ll += log(r) + 0.0 * log(t);
                g += 0.0 / t;
            }
        } else {
            const double r = p * qj;
            const double t = 1.0 - r;
            ll += exact ? 0.0 * log(r) + log(t) : log(t);
            g += qj / t;
        }
    }
    const size_t o = (size_t)slab * G + i;
    dp_part[o] = g;
    ll_part[o] = ll;
    cnt_part[o] = cnt;
}

__global__ __launch_bounds__(BN_THREADS) void bern_cols_kernel(const unsigned long long *__restrict__ bits,
                                                               uint32_t stride, uint32_t G, uint32_t S,
                                                               const double *__restrict__ pq, uint32_t words,
                                                               uint32_t span, const uint32_t *__restrict__ mode,
                                                               double *__restrict__ dq_part, uint32_t *__restrict__ cnt_part) {
#pragma clang fp contract(off)
    const uint32_t j = blockIdx.x * BN_THREADS + threadIdx.x;
    if (j >= S) return;
    const uint32_t slab = blockIdx.y;
    const uint32_t w0 = slab * span, w1 = min(words, w0 + span);
    const bool exact = mode[0] != 0;
    const double qj = pq[G + j];
    double g = 0.0;
    uint32_t cnt = 0;
    for (uint32_t w = w0; w < w1; ++w) {
        const uint32_t base = w * 64;
        const uint32_t nb = min(64u, G - base);                 // pad bits beyond G are not cells
        const unsigned long long valid = nb == 64 ? ~0ull : ((1ull << nb) - 1ull);
        const unsigned long long word = bits[(size_t)j * stride + w] & valid;
        cnt += (uint32_t)__popcll(word);
        if (exact) {
            for (uint32_t b = 0; b < nb; ++b) {
                const double pi = pq[base + b];
                const double t = 1.0 - pi * qj;
                g += ((word >> b) & 1ull) ? 0.0 / t : pi / t;
            }
        } else {
            // present cells add exactly 0 here: only the absent ones, in ascending gene order
            for (unsigned long long z = ~word & valid; z; z &= z - 1ull) {
                const uint32_t b = (uint32_t)__builtin_ctzll(z);
                const double pi = pq[base + b];
                const double t = 1.0 - pi * qj;
                g += pi / t;
            }
        }
    }
    const size_t o = (size_t)slab * S + j;
    dq_part[o] = g;
    cnt_part[o] = cnt;
}

// out = [LL, dL/dp (G), dL/dq (S)]; terms[k] = row k's (k < G) or column k - G's share of LL
__global__ __launch_bounds__(BN_THREADS) void bern_fold_kernel(uint32_t G, uint32_t S, const double *__restrict__ pq,
                                                               uint32_t a_slabs, uint32_t b_slabs,
                                                               const uint32_t *__restrict__ mode,
                                                               const double *__restrict__ dp_part,
                                                               const double *__restrict__ ll_part,
                                                               const uint32_t *__restrict__ cnt_a,
                                                               const double *__restrict__ dq_part,
                                                               const uint32_t *__restrict__ cnt_b,
                                                               double *__restrict__ out, double *__restrict__ terms) {
#pragma clang fp contract(off)
    const uint32_t k = blockIdx.x * BN_THREADS + threadIdx.x;
    if (k >= G + S) return;
    const bool fast = mode[0] == 0;
    double g = 0.0, ll = 0.0;
    uint64_t cnt = 0;
    if (k < G) {
        for (uint32_t s = 0; s < a_slabs; ++s) {
            const size_t o = (size_t)s * G + k;
            g += dp_part[o];
            ll += ll_part[o];
            cnt += cnt_a[o];
        }
    } else {
        for (uint32_t s = 0; s < b_slabs; ++s) {
            const size_t o = (size_t)s * S + (k - G);
            g += dq_part[o];
            cnt += cnt_b[o];
        }
    }
    const double v = pq[k];
    out[1 + k] = (double)cnt / v - g;
    if (fast && cnt) ll += (double)cnt * log(v);
    terms[k] = ll;
}

__global__ __launch_bounds__(1024) void bern_total_kernel(const double *__restrict__ terms, uint32_t n,
                                                          double *__restrict__ out) {
    __shared__ double s[1024];
    double v = 0.0;
    for (uint32_t k = threadIdx.x; k < n; k += 1024) v += terms[k];
    s[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t d = 512; d > 0; d >>= 1) {
        if (threadIdx.x < d) s[threadIdx.x] += s[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = s[0];
}

int eval_dev(pgx_ctx *ctx, const uint64_t *d_bits, uint32_t G, uint32_t S, const double *d_pq, uint32_t flags,
             double *d_out, void *d_ws, size_t ws_bytes, void *stream_) {
    PGX_REQUIRE(ctx, "NULL context");
    PGX_REQUIRE(d_pq && d_out && d_ws && (d_bits || G == 0 || S == 0), "NULL argument");
    PGX_REQUIRE((uint64_t)G + S < (1ull << 31), "table too large");
    PGX_REQUIRE((flags & ~(uint32_t)PGX_BERNOULLI_EXACT) == 0, "unknown flag");
    const BernGeom g = make_geom(G, S);
    PGX_REQUIRE(ws_bytes >= g.bytes, "workspace too small (see pgx_bernoulli_workspace_bytes)");
    hipStream_t stream = (hipStream_t)stream_;
    char *ws = (char *)d_ws;
    uint32_t *mode = (uint32_t *)ws;
    double *dp = (double *)(ws + g.off_dp), *ll = (double *)(ws + g.off_ll), *dq = (double *)(ws + g.off_dq);
    uint32_t *cnt_a = (uint32_t *)(ws + g.off_cnt_a), *cnt_b = (uint32_t *)(ws + g.off_cnt_b);
    double *terms = (double *)(ws + g.off_terms);
    {
        ProfScope prof(ctx, "bern_mode_kernel", stream);
        bern_mode_kernel<<<1, 1024, 0, stream>>>(d_pq, G, S, (flags & PGX_BERNOULLI_EXACT) ? 1u : 0u, mode);
    }
    PGX_HIP(hipGetLastError());
    if (G && S) {
        {
            ProfScope prof(ctx, "bern_rows_kernel", stream);
            bern_rows_kernel<<<dim3(ceil_div_u32(G, BN_THREADS), g.a_slabs), BN_THREADS, 0, stream>>>(
                (const unsigned long long *)d_bits, g.stride, G, S, d_pq, g.a_span, mode, dp, ll, cnt_a);
        }
        PGX_HIP(hipGetLastError());
        {
            ProfScope prof(ctx, "bern_cols_kernel", stream);
            bern_cols_kernel<<<dim3(ceil_div_u32(S, BN_THREADS), g.b_slabs), BN_THREADS, 0, stream>>>(
                (const unsigned long long *)d_bits, g.stride, G, S, d_pq, g.words, g.b_span, mode, dq, cnt_b);
        }
        PGX_HIP(hipGetLastError());
    } else {   // an empty table: every sum is empty
        PGX_HIP(hipMemsetAsync(ws + g.off_dp, 0, g.bytes - g.off_dp, stream));
    }
    if (G + S) {
        ProfScope prof(ctx, "bern_fold_kernel", stream);
        bern_fold_kernel<<<ceil_div_u32(G + S, BN_THREADS), BN_THREADS, 0, stream>>>(
            G, S, d_pq, g.a_slabs, g.b_slabs, mode, dp, ll, cnt_a, dq, cnt_b, d_out, terms);
        PGX_HIP(hipGetLastError());
    }
    {
        ProfScope prof(ctx, "bern_total_kernel", stream);
        bern_total_kernel<<<1, 1024, 0, stream>>>(terms, G + S, d_out);
    }
    PGX_HIP(hipGetLastError());
    return PGX_OK;
}

int load_coo(pgx_ctx *ctx, const int32_t *rows, const int32_t *genomes, uint64_t n_records, uint32_t G, uint32_t S,
             uint64_t *out_duplicates) {
    PGX_REQUIRE(ctx, "NULL context");
    PGX_REQUIRE(n_records == 0 || (rows && genomes), "NULL record arrays");
    PGX_REQUIRE((uint64_t)G + S < (1ull << 31), "table too large");
    PGX_HIP(hipSetDevice(ctx->device_id));
    ctx->bern_loaded = false;
    DevBuf d_bits(ctx, PGX_SLOT_BERN_BITS), d_cnt(ctx, BN_SLOT_CNT);
    const int rc = pgx_load_coo_bitmap(ctx, rows, genomes, n_records, G, S, BN_SLOT_ROWS, BN_SLOT_GENOMES, d_bits, d_cnt,
                                       out_duplicates);
    if (rc != PGX_OK) return rc;
    ctx->bern_genes = G;
    ctx->bern_genomes = S;
    ctx->bern_loaded = true;
    return PGX_OK;
}

int load_resident(pgx_ctx *ctx, uint64_t token, const int32_t *row_map, uint32_t G, uint32_t S) {
    PGX_REQUIRE(ctx, "NULL context");
    PGX_REQUIRE(G == 0 || row_map, "NULL row map");
    ResidentBitmap src;
    int rc = pgx_resident_bitmap(ctx, token, S, &src);
    if (rc != PGX_OK) return rc;
    PGX_REQUIRE((uint64_t)G + S < (1ull << 31), "table too large");
    PGX_HIP(hipSetDevice(ctx->device_id));
    DevBuf d_map(ctx, BN_SLOT_MAP), d_bits(ctx, PGX_SLOT_BERN_BITS);
    rc = pgx_gather_resident(ctx, src, row_map, nullptr, G, S, d_map, nullptr, d_bits, "bern_gather_rows_kernel");
    if (rc != PGX_OK && rc != PGX_ERR_INVALID) ctx->bern_loaded = false;   // (a refused map leaves the loaded table alone)
    if (rc != PGX_OK) return rc;
    ctx->bern_genes = G;
    ctx->bern_genomes = S;
    ctx->bern_loaded = true;
    return PGX_OK;
}

int eval_loaded(pgx_ctx *ctx, const double *pq, uint32_t flags, double *out) {
    PGX_REQUIRE(ctx && pq && out, "NULL argument");
    PGX_REQUIRE(ctx->bern_loaded, "no table loaded (pgx_bernoulli_load / pgx_bernoulli_load_resident)");
    PGX_HIP(hipSetDevice(ctx->device_id));
    const uint32_t G = ctx->bern_genes, S = ctx->bern_genomes;
    const size_t n = (size_t)G + S;
    const size_t nws = make_geom(G, S).bytes;
    DevBuf d_bits(ctx, PGX_SLOT_BERN_BITS), d_pq(ctx, BN_SLOT_PQ), d_out(ctx, BN_SLOT_OUT), d_ws(ctx, BN_SLOT_WS);
    int rc = d_bits.view((size_t)S * pgx_bitmap_stride_words(G) * 8);    // (the loaded table)
    if (rc != PGX_OK) return rc;
    PGX_HIP(d_pq.alloc(n * 8));
    PGX_HIP(d_out.alloc((n + 1) * 8));
    PGX_HIP(d_ws.alloc(nws));
    if (n) PGX_HIP(hipMemcpyAsync(d_pq.p, pq, n * 8, hipMemcpyHostToDevice, ctx->stream));
    rc = eval_dev(ctx, d_bits.as<uint64_t>(), G, S, d_pq.as<double>(), flags, d_out.as<double>(), d_ws.p, nws, ctx->stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(hipMemcpyAsync(out, d_out.p, (n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    PGX_HIP(hipStreamSynchronize(ctx->stream));
    return PGX_OK;
}

}  // namespace

extern "C" {

size_t pgx_bernoulli_workspace_bytes(uint32_t n_genes, uint32_t n_genomes) {
    try {
        return make_geom(n_genes, n_genomes).bytes;
    } catch (...) {
        return 0;
    }
}

int pgx_bernoulli_eval_dev(pgx_ctx *ctx, const uint64_t *d_bits, uint32_t n_genes, uint32_t n_genomes, const double *d_pq,
                           uint32_t flags, double *d_out, void *d_workspace, size_t workspace_bytes, void *stream) {
    return guarded(__func__, [&] {
        return eval_dev(ctx, d_bits, n_genes, n_genomes, d_pq, flags, d_out, d_workspace, workspace_bytes, stream);
    });
}

int pgx_bernoulli_load(pgx_ctx *ctx, const int32_t *rows, const int32_t *genomes, uint64_t n_records, uint32_t n_genes,
                       uint32_t n_genomes, uint64_t *out_duplicates) {
    return guarded(__func__, [&] { return load_coo(ctx, rows, genomes, n_records, n_genes, n_genomes, out_duplicates); });
}

int pgx_bernoulli_load_resident(pgx_ctx *ctx, uint64_t token, const int32_t *row_map, uint32_t n_genes,
                                uint32_t n_genomes) {
    return guarded(__func__, [&] { return load_resident(ctx, token, row_map, n_genes, n_genomes); });
}

int pgx_bernoulli_eval(pgx_ctx *ctx, const double *pq, uint32_t flags, double *out) {
    return guarded(__func__, [&] { return eval_loaded(ctx, pq, flags, out); });
}

}  // extern "C"
