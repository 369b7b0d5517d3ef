// A bagged ensemble of linear SVMs trained in the dual on the genome-major bitmap (reference ml_pipelines.py
// evaluate_model: sklearn BaggingClassifier(LinearSVC) on genomes x blocks). The samples are the genomes,
// the features the rows of the table. One SUB-PROBLEM p = {a feature mask, a multiplicity m_i per genome (bootstrap draws
// folded; 0 = not in the training set), C}; labels y_i in {0, 1} -> -1 / +1. With the copies of a genome summed into one
// variable, the dual of LinearSVC(l2, squared_hinge, fit_intercept, intercept_scaling = 1) is
//      min 1/2 b'Qb - sum b_i,  b >= 0,   Q_ij = y_i y_j (K_ij + 1) + [i == j] / (2 C m_i),   K_ij = popcount(bits_i & bits_j & mask)
// over the genomes with m_i > 0. Q is positive definite, the optimum unique.
//
// Kernels (plain launches on one stream, no workgroup waits for another, no floating-point atomic):
//   svm_check_kernel   one wave per sub-problem, then one per mask: the rules of pgx.h, ORed into a status word (integer)
//   svm_gram_kernel    per mask the whole n x n matrix K (uint32, exact): 32 x 32 tiles, 256 threads with 2 x 2 entries
//                      each, 16 words of the masked rows at a time through LDS (rows padded by one word: the 16 rows a
//                      wave reads lie on 16 different bank pairs). Only tiles on or below the diagonal run; each stores
//                      its mirror image too.
//   svm_solve_kernel   ONE WAVE per sub-problem: greedy dual coordinate descent in double precision (the rule is pinned
//                      in pgx.h). g, b, the multiplicities and the signs live in LDS, lane l owns the genomes l, l + 64,
//                      ...; a step reads row i of K (from the L2 where members share a mask), updates g and finds the next largest |projected
//                      gradient| in the same pass, then a 6-stage xor butterfly of (value, index) over the wave -- ties
//                      go to the smaller index at every stage, so the pick does not depend on the lanes. A workgroup
//                      of one wave needs no hardware barrier: its __syncthreads() only orders the LDS traffic.
//                      When the test passes, g and the decisions of EVERY genome are recomputed from b in ascending
//                      order of i and the test is repeated on that g.
//   svm_coef_kernel    one thread per (sub-problem, row): coef[r] = sum over the genomes ascending of b_i y_i bit(i, r);
//                      the 64 lanes of a wave are 64 neighbouring rows = one word of the bitmap per genome.
// The same inputs give the same bits: every sum runs in a fixed order and every maximum breaks ties by index.
#include "pgx_internal.h"

#include <cmath>

namespace {

constexpr int SV_TILE = 32, SV_WORDS = 16, SV_GRAM_THREADS = 256, SV_COEF_THREADS = 256;
constexpr uint32_t SV_ERR_MASK_INDEX = 1u, SV_ERR_MASK_EMPTY = 2u, SV_ERR_C = 4u, SV_ERR_ONE_CLASS = 8u, SV_ERR_LABEL = 16u,
                   SV_ERR_STEPS = 32u;
constexpr uint32_t SV_NONE = 0xFFFFFFFFu;

struct SvmGeom {
    uint32_t stride;
    size_t off_gram, off_status, bytes;
};

bool sizes_ok(uint32_t n_rows, uint32_t n_genomes, uint32_t n_masks, uint32_t n_problems) {
    return n_rows < (1u << 30) && n_genomes <= PGX_SVM_MAX_GENOMES && n_masks <= 65535u && n_problems <= 65535u;
}

SvmGeom make_geom(uint32_t n_rows, uint32_t n_genomes, uint32_t n_masks) {
    SvmGeom g;
    g.stride = pgx_bitmap_stride_words(n_rows);
    WsLayout ws;
    g.off_gram = ws.take((size_t)n_masks * n_genomes * n_genomes * 4);
    g.off_status = ws.take(16);
    g.bytes = ws.off;
    return g;
}

// max_steps = 0 (pgx.h)
uint32_t default_max_steps(uint32_t n_genomes) { return 1000000u + 2000u * n_genomes; }

// bytes of LDS the solver takes for n genomes: g, b (double), multiplicities (uint16), signs (int8)
size_t solve_lds_bytes(uint32_t n) {
    const size_t npad = ((size_t)n + 63) & ~(size_t)63;
    return npad * (8 + 8 + 2 + 1);
}

__device__ __forceinline__ bool finite_positive(double x) { return x > 0.0 && x < __builtin_huge_val(); }

// blocks [0, n_problems): the sub-problem's mask index, C, labels, and that its drawn genomes carry both classes;
// blocks [n_problems, n_problems + n_masks): the mask has a bit among the n_rows rows.
__global__ __launch_bounds__(64) void svm_check_kernel(const unsigned long long *__restrict__ masks, uint32_t n_masks,
                                                       uint32_t stride, uint32_t n_rows,
                                                       const int32_t *__restrict__ mask_of, const double *__restrict__ Cs,
                                                       const uint16_t *__restrict__ mult, uint32_t n_problems,
                                                       const uint8_t *__restrict__ labels, uint32_t n,
                                                       uint32_t *__restrict__ status) {
    const uint32_t lane = threadIdx.x;
    uint32_t err = 0;
    if (blockIdx.x < n_problems) {
        const uint32_t p = blockIdx.x;
        if (lane == 0) {
            const int32_t mi = mask_of[p];
            if (mi < 0 || (uint32_t)mi >= n_masks) err |= SV_ERR_MASK_INDEX;
            if (!finite_positive(Cs[p])) err |= SV_ERR_C;
        }
        bool pos = false, neg = false;
        for (uint32_t j = lane; j < n; j += 64u) {
            const uint8_t y = labels[j];
            if (y > 1u) err |= SV_ERR_LABEL;
            if (mult[(size_t)p * n + j]) {
                if (y) pos = true;
                else neg = true;
            }
        }
        const bool both = __any(pos) && __any(neg);             // (every lane votes: not under the lane test)
        if (lane == 0 && !both) err |= SV_ERR_ONE_CLASS;
    } else {
        const uint32_t t = blockIdx.x - n_problems;
        const uint32_t words = (n_rows + 63u) / 64u;
        bool any = false;
        for (uint32_t w = lane; w < words; w += 64u) {
            unsigned long long m = masks[(size_t)t * stride + w];
            if (w == words - 1u && (n_rows & 63u)) m &= (1ull << (n_rows & 63u)) - 1ull;
            any |= m != 0ull;
        }
        const bool some = __any(any);
        if (lane == 0 && !some) err |= SV_ERR_MASK_EMPTY;
    }
    if (err) atomicOr(status, err);
}

// K[t][a][b] = popcount(bits[a] & bits[b] & mask[t]) over the stride words, a >= b computed, both stored.
__global__ __launch_bounds__(SV_GRAM_THREADS) void svm_gram_kernel(const unsigned long long *__restrict__ bits,
                                                                   const unsigned long long *__restrict__ masks,
                                                                   uint32_t stride, uint32_t n, uint32_t *__restrict__ gram) {
    if (blockIdx.x > blockIdx.y) return;                          // (the tile above the diagonal is its mirror's)
    __shared__ unsigned long long A[SV_TILE][SV_WORDS + 1], B[SV_TILE][SV_WORDS + 1];
    const uint32_t tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
    const uint32_t a0 = blockIdx.y * SV_TILE, b0 = blockIdx.x * SV_TILE;
    const unsigned long long *mask = masks + (size_t)blockIdx.z * stride;
    uint32_t c00 = 0, c01 = 0, c10 = 0, c11 = 0;
    for (uint32_t w0 = 0; w0 < stride; w0 += SV_WORDS) {          // (stride is a multiple of 16 words)
        for (uint32_t e = threadIdx.x; e < SV_TILE * SV_WORDS; e += SV_GRAM_THREADS) {
            const uint32_t row = e >> 4, w = e & 15u;
            const unsigned long long mw = mask[w0 + w];
            A[row][w] = a0 + row < n ? bits[(size_t)(a0 + row) * stride + w0 + w] & mw : 0ull;
            B[row][w] = b0 + row < n ? bits[(size_t)(b0 + row) * stride + w0 + w] : 0ull;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t w = 0; w < SV_WORDS; ++w) {
            const unsigned long long x0 = A[ty][w], x1 = A[ty + 16][w], y0 = B[tx][w], y1 = B[tx + 16][w];
            c00 += (uint32_t)__popcll(x0 & y0);
            c01 += (uint32_t)__popcll(x0 & y1);
            c10 += (uint32_t)__popcll(x1 & y0);
            c11 += (uint32_t)__popcll(x1 & y1);
        }
        __syncthreads();
    }
    uint32_t *K = gram + (size_t)blockIdx.z * n * n;
    const uint32_t a[2] = {a0 + ty, a0 + ty + 16u}, b[2] = {b0 + tx, b0 + tx + 16u};
    const uint32_t c[2][2] = {{c00, c01}, {c10, c11}};
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
            if (a[i] < n && b[j] < n) {
                K[(size_t)a[i] * n + b[j]] = c[i][j];
                K[(size_t)b[j] * n + a[i]] = c[i][j];
            }
}

// (largest value, smallest index among equals) over the wave; every lane gets the result
__device__ __forceinline__ void wave_argmax(double &best, uint32_t &bi) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(best, off, 64);
        const uint32_t oi = (uint32_t)__shfl_xor((int)bi, off, 64);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
}

__device__ __forceinline__ double projected_abs(double g, double b) { return fabs(b > 0.0 ? g : fmin(g, 0.0)); }

__global__ __launch_bounds__(64) void svm_solve_kernel(const uint32_t *__restrict__ gram, const int32_t *__restrict__ mask_of,
                                                       uint32_t n_masks, const double *__restrict__ Cs,
                                                       const uint16_t *__restrict__ mult, const uint8_t *__restrict__ labels,
                                                       uint32_t n, double tol, uint32_t max_steps, double *__restrict__ out_beta,
                                                       double *__restrict__ out_intercept, double *__restrict__ out_decision,
                                                       uint32_t *__restrict__ out_steps, uint32_t *__restrict__ status) {
    extern __shared__ __align__(16) unsigned char sv_lds[];
    const uint32_t npad = (n + 63u) & ~63u;
    double *g = (double *)sv_lds, *beta = g + npad;
    uint16_t *m = (uint16_t *)(beta + npad);
    signed char *ys = (signed char *)(m + npad);
    const uint32_t p = blockIdx.x, lane = threadIdx.x;
    const int32_t mi = mask_of[p];
    const double C = Cs[p];
    if (mi < 0 || (uint32_t)mi >= n_masks || !finite_positive(C)) {       // (reported by svm_check_kernel; nothing is read)
        if (lane == 0) { out_steps[p] = 0u; out_intercept[p] = 0.0; }
        for (uint32_t j = lane; j < n; j += 64u) out_beta[(size_t)p * n + j] = out_decision[(size_t)p * n + j] = 0.0;
        return;
    }
    const uint32_t *K = gram + (size_t)mi * n * n;
    for (uint32_t j = lane; j < npad; j += 64u) {
        const uint16_t mj = j < n ? mult[(size_t)p * n + j] : (uint16_t)0;
        m[j] = mj;
        ys[j] = mj ? (labels[j] ? 1 : -1) : 0;
        beta[j] = 0.0;
        g[j] = -1.0;
    }
    __syncthreads();
    double best = 0.0;
    uint32_t bi = SV_NONE;
    for (uint32_t j = lane; j < n; j += 64u)
        if (ys[j]) {
            const double a = projected_abs(g[j], beta[j]);
            if (a > best) { best = a; bi = j; }
        }
    wave_argmax(best, bi);
    uint32_t steps = 0;
    bool failed = false;
    for (;;) {
        if (!(best > tol)) {
            // g and the decisions of all genomes from b alone, i ascending: dec_s = sum b_i y_i (K_si + 1)
            best = 0.0;
            bi = SV_NONE;
            for (uint32_t s = lane; s < n; s += 64u) {
                double dec = 0.0;
                for (uint32_t i = 0; i < n; ++i) {
                    const double b = beta[i];
                    if (b != 0.0) dec += b * (double)ys[i] * (double)(K[(size_t)i * n + s] + 1u);
                }
                out_decision[(size_t)p * n + s] = dec;
                if (ys[s]) {
                    const double gs = (double)ys[s] * dec + beta[s] / (2.0 * C * (double)m[s]) - 1.0;
                    g[s] = gs;
                    const double a = projected_abs(gs, beta[s]);
                    if (a > best) { best = a; bi = s; }
                }
            }
            wave_argmax(best, bi);
            __syncthreads();
            if (!(best > tol)) break;
        }
        if (steps >= max_steps) { failed = true; break; }
        const uint32_t i = bi;                                    // (uniform; an active genome: best > 0)
        const double diag = 1.0 / (2.0 * C * (double)m[i]);
        const double qii = (double)(K[(size_t)i * n + i] + 1u) + diag;
        const double bi_old = beta[i];
        const double d = fmax(-bi_old, -g[i] / qii);
        const double bi_new = bi_old + d;
        const double yi = (double)ys[i];
        __syncthreads();                                          // (every lane has read g[i] and beta[i])
        best = 0.0;
        bi = SV_NONE;
        for (uint32_t j = lane; j < n; j += 64u) {
            const signed char yj = ys[j];
            if (!yj) continue;
            double q = (double)yj * yi * (double)(K[(size_t)i * n + j] + 1u);
            double bj = beta[j];
            if (j == i) { q += diag; bj = bi_new; beta[j] = bi_new; }
            const double gj = g[j] + d * q;
            g[j] = gj;
            const double a = projected_abs(gj, bj);
            if (a > best) { best = a; bi = j; }
        }
        wave_argmax(best, bi);
        __syncthreads();
        ++steps;
    }
    for (uint32_t j = lane; j < n; j += 64u) out_beta[(size_t)p * n + j] = ys[j] ? beta[j] : 0.0;
    if (lane == 0) {
        double b0 = 0.0;
        for (uint32_t i = 0; i < n; ++i)
            if (ys[i]) b0 += beta[i] * (double)ys[i];
        out_intercept[p] = b0;
        out_steps[p] = steps;
        if (failed) atomicOr(status, SV_ERR_STEPS);
    }
}

// coef[p][r] = sum_i b_i y_i bit(i, r) for the rows of p's mask, i ascending; 0 outside the mask
__global__ __launch_bounds__(SV_COEF_THREADS) void svm_coef_kernel(const unsigned long long *__restrict__ bits,
                                                                   const unsigned long long *__restrict__ masks,
                                                                   uint32_t stride, uint32_t n_rows, uint32_t n,
                                                                   const int32_t *__restrict__ mask_of, uint32_t n_masks,
                                                                   const double *__restrict__ beta,
                                                                   const uint8_t *__restrict__ labels, double *__restrict__ coef) {
    const uint32_t p = blockIdx.y, r = blockIdx.x * SV_COEF_THREADS + threadIdx.x;
    if (r >= n_rows) return;
    const int32_t mi = mask_of[p];
    double acc = 0.0;
    if (mi >= 0 && (uint32_t)mi < n_masks && ((masks[(size_t)mi * stride + (r >> 6)] >> (r & 63u)) & 1ull)) {
        const unsigned long long *col = bits + (r >> 6);
        const double *b = beta + (size_t)p * n;
        for (uint32_t i = 0; i < n; ++i) {
            const double w = b[i];                                // (uniform over the workgroup)
            if (w == 0.0) continue;
            if ((col[(size_t)i * stride] >> (r & 63u)) & 1ull) acc += labels[i] ? w : -w;
        }
    }
    coef[(size_t)p * n_rows + r] = acc;
}

const char *status_error(uint32_t s) {
    if (s & SV_ERR_MASK_INDEX) return "mask index out of range";
    if (s & SV_ERR_MASK_EMPTY) return "a mask without a feature";
    if (s & SV_ERR_C) return "C must be finite and positive";
    if (s & SV_ERR_LABEL) return "labels must be 0 or 1";
    if (s & SV_ERR_ONE_CLASS) return "a sub-problem whose drawn genomes carry one class only";
    return nullptr;
}

int scalars_ok(pgx_ctx *ctx, uint32_t n_rows, uint32_t n_genomes, uint32_t n_masks, uint32_t n_problems, double tol) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(n_rows && n_genomes && n_problems && n_masks, "n_rows, n_genomes, n_masks and n_problems must be positive");
    PGX_REQUIRE(tol > 0.0 && std::isfinite(tol), "tol must be finite and positive");
    if (n_genomes > PGX_SVM_MAX_GENOMES) {
        pgx_set_error("pgx_svm_bag: %u genomes, at most %u are supported", n_genomes, PGX_SVM_MAX_GENOMES);
        return PGX_ERR_CAPACITY;
    }
    PGX_REQUIRE(sizes_ok(n_rows, n_genomes, n_masks, n_problems), "table, masks or sub-problems too many");
    return PGX_OK;
}

// Everything on the device; `stream` is synchronised once at the end (the status word is read back).
int svm_run(pgx_ctx *ctx, const uint64_t *d_bits, uint32_t n_rows, uint32_t n_genomes, const uint64_t *d_masks,
            uint32_t n_masks, const int32_t *d_mask_of, const double *d_C, const uint16_t *d_mult, uint32_t n_problems,
            const uint8_t *d_labels, double tol, uint32_t max_steps, double *d_beta, double *d_coef, double *d_intercept,
            double *d_decision, uint32_t *d_steps, void *d_ws, size_t ws_bytes, hipStream_t stream) {
    const int rc = scalars_ok(ctx, n_rows, n_genomes, n_masks, n_problems, tol);
    if (rc != PGX_OK) return rc;
    PGX_REQUIRE(d_bits && d_masks && d_mask_of && d_C && d_mult && d_labels && d_beta && d_coef && d_intercept && d_decision &&
                    d_steps && d_ws,
                "NULL argument");
    const SvmGeom g = make_geom(n_rows, n_genomes, n_masks);
    PGX_REQUIRE(ws_bytes >= g.bytes, "workspace too small (see pgx_svm_bag_workspace_bytes)");
    PGX_REQUIRE(((uintptr_t)d_ws & 15u) == 0, "workspace must be 16-byte aligned");
    if (!max_steps) max_steps = default_max_steps(n_genomes);
    HostVec<uint32_t> h_status(ctx, SV_HOST_STATUS, 4);
    if (!h_status.ok()) { pgx_set_error("%s: out of page-locked host memory", __func__); return PGX_ERR_NOMEM; }
    const size_t lds = solve_lds_bytes(n_genomes);
    if (lds > 48u * 1024u)
        PGX_HIP(hipFuncSetAttribute((const void *)svm_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    uint32_t *gram = (uint32_t *)((char *)d_ws + g.off_gram), *status = (uint32_t *)((char *)d_ws + g.off_status);
    const unsigned long long *bits = (const unsigned long long *)d_bits, *masks = (const unsigned long long *)d_masks;
    const uint32_t tiles = ceil_div_u32(n_genomes, SV_TILE);

    PGX_HIP(hipMemsetAsync(status, 0, 16, stream));
    {
        ProfScope prof(ctx, "svm_check_kernel", stream);
        svm_check_kernel<<<n_problems + n_masks, 64, 0, stream>>>(masks, n_masks, g.stride, n_rows, d_mask_of, d_C, d_mult,
                                                                  n_problems, d_labels, n_genomes, status);
    }
    PGX_HIP(hipGetLastError());
    {
        ProfScope prof(ctx, "svm_gram_kernel", stream);
        svm_gram_kernel<<<dim3(tiles, tiles, n_masks), SV_GRAM_THREADS, 0, stream>>>(bits, masks, g.stride, n_genomes, gram);
    }
    PGX_HIP(hipGetLastError());
    {
        ProfScope prof(ctx, "svm_solve_kernel", stream);
        svm_solve_kernel<<<n_problems, 64, lds, stream>>>(gram, d_mask_of, n_masks, d_C, d_mult, d_labels, n_genomes, tol,
                                                          max_steps, d_beta, d_intercept, d_decision, d_steps, status);
    }
    PGX_HIP(hipGetLastError());
    {
        ProfScope prof(ctx, "svm_coef_kernel", stream);
        svm_coef_kernel<<<dim3(ceil_div_u32(n_rows, SV_COEF_THREADS), n_problems), SV_COEF_THREADS, 0, stream>>>(
            bits, masks, g.stride, n_rows, n_genomes, d_mask_of, n_masks, d_beta, d_labels, d_coef);
    }
    PGX_HIP(hipGetLastError());
    PGX_HIP(hipMemcpyAsync(h_status.data(), status, 4, hipMemcpyDeviceToHost, stream));
    PGX_HIP(hipStreamSynchronize(stream));
    const char *why = status_error(h_status[0]);
    PGX_REQUIRE(!why, why);
    if (h_status[0] & SV_ERR_STEPS) {
        pgx_set_error("%s: a sub-problem needs more than %u steps", __func__, max_steps);
        return PGX_ERR_INTERNAL;
    }
    return PGX_OK;
}

// The rules of pgx.h on host arrays, before anything is launched.
int svm_host_check(const uint64_t *masks, uint32_t n_masks, uint32_t n_rows, const int32_t *mask_of, const double *C,
                   const uint16_t *mult, uint32_t n_problems, const uint8_t *labels, uint32_t n) {
    const uint32_t stride = pgx_bitmap_stride_words(n_rows), words = (n_rows + 63u) / 64u;
    for (uint32_t j = 0; j < n; ++j) PGX_REQUIRE(labels[j] <= 1u, "labels must be 0 or 1");
    for (uint32_t t = 0; t < n_masks; ++t) {
        uint64_t any = 0;
        for (uint32_t w = 0; w < words; ++w) {
            uint64_t mw = masks[(size_t)t * stride + w];
            if (w == words - 1u && (n_rows & 63u)) mw &= (1ull << (n_rows & 63u)) - 1ull;
            any |= mw;
        }
        PGX_REQUIRE(any != 0, "a mask without a feature");
    }
    for (uint32_t p = 0; p < n_problems; ++p) {
        PGX_REQUIRE(mask_of[p] >= 0 && (uint32_t)mask_of[p] < n_masks, "mask index out of range");
        PGX_REQUIRE(C[p] > 0.0 && std::isfinite(C[p]), "C must be finite and positive");
        bool pos = false, neg = false;
        for (uint32_t j = 0; j < n; ++j)
            if (mult[(size_t)p * n + j]) (labels[j] ? pos : neg) = true;
        PGX_REQUIRE(pos && neg, "a sub-problem whose drawn genomes carry one class only");
    }
    return PGX_OK;
}

int svm_host(pgx_ctx *ctx, const int32_t *rows, const int32_t *genomes, uint64_t n_records, uint32_t n_rows,
             uint32_t n_genomes, const uint64_t *masks, uint32_t n_masks, const int32_t *mask_of, const double *C,
             const uint16_t *mult, uint32_t n_problems, const uint8_t *labels, double tol, uint32_t max_steps,
             double *out_beta, double *out_coef, double *out_intercept, double *out_decision, uint32_t *out_steps) {
    int rc = scalars_ok(ctx, n_rows, n_genomes, n_masks, n_problems, tol);
    if (rc != PGX_OK) return rc;
    PGX_REQUIRE(n_records == 0 || (rows && genomes), "NULL record arrays");
    PGX_REQUIRE(masks && mask_of && C && mult && labels && out_beta && out_coef && out_intercept && out_decision && out_steps,
                "NULL argument");
    rc = svm_host_check(masks, n_masks, n_rows, mask_of, C, mult, n_problems, labels, n_genomes);
    if (rc != PGX_OK) return rc;
    PGX_HIP(hipSetDevice(ctx->device_id));
    hipStream_t stream = ctx->stream;
    DevBuf d_bits(ctx, SV_SLOT_BITS), d_cnt(ctx, SV_SLOT_CNT);
    uint64_t dup = 0;
    rc = pgx_load_coo_bitmap(ctx, rows, genomes, n_records, n_rows, n_genomes, SV_SLOT_ROWS, SV_SLOT_GENOMES, d_bits, d_cnt, &dup);
    if (rc != PGX_OK) return rc;
    PGX_REQUIRE(dup == 0, "duplicate coordinates: not a 0/1 table");
    const SvmGeom g = make_geom(n_rows, n_genomes, n_masks);
    const size_t n = n_genomes, P = n_problems;
    DevBuf d_ws(ctx, SV_SLOT_WS);
    DevPack in(ctx, SV_SLOT_IN), res(ctx, SV_SLOT_OUT);
    const PackPart i_masks = in.in(masks, (size_t)n_masks * g.stride), i_mask_of = in.in(mask_of, P), i_C = in.in(C, P),
                   i_mult = in.in(mult, P * n), i_labels = in.in(labels, n);
    const PackPart o_beta = res.out(out_beta, P * n), o_coef = res.out(out_coef, P * n_rows), o_icpt = res.out(out_intercept, P),
                   o_dec = res.out(out_decision, P * n), o_steps = res.out(out_steps, P);
    PGX_HIP(d_ws.alloc(g.bytes));
    PGX_HIP(in.alloc());
    PGX_HIP(res.alloc());
    PGX_HIP(in.upload(stream));
    rc = svm_run(ctx, d_bits.as<uint64_t>(), n_rows, n_genomes, in.dev<uint64_t>(i_masks), n_masks, in.dev<int32_t>(i_mask_of),
                 in.dev<double>(i_C), in.dev<uint16_t>(i_mult), n_problems, in.dev<uint8_t>(i_labels), tol, max_steps,
                 res.dev<double>(o_beta), res.dev<double>(o_coef), res.dev<double>(o_icpt), res.dev<double>(o_dec),
                 res.dev<uint32_t>(o_steps), d_ws.p, g.bytes, stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(res.download(stream));
    PGX_HIP(hipStreamSynchronize(stream));
    return PGX_OK;
}

}  // namespace

extern "C" {

size_t pgx_svm_bag_workspace_bytes(uint32_t n_rows, uint32_t n_genomes, uint32_t n_masks) {
    if (!sizes_ok(n_rows, n_genomes, n_masks, 0)) return 0;
    return make_geom(n_rows, n_genomes, n_masks).bytes;
}

int pgx_svm_bag(pgx_ctx *ctx, const int32_t *rows, const int32_t *genomes, uint64_t n_records, uint32_t n_rows,
                uint32_t n_genomes, const uint64_t *masks, uint32_t n_masks, const int32_t *mask_of_problem, const double *C,
                const uint16_t *multiplicity, uint32_t n_problems, const uint8_t *labels, double tol, uint32_t max_steps,
                double *out_beta, double *out_coef, double *out_intercept, double *out_decision, uint32_t *out_steps) {
    return guarded(__func__, [&] {
        return svm_host(ctx, rows, genomes, n_records, n_rows, n_genomes, masks, n_masks, mask_of_problem, C, multiplicity,
                        n_problems, labels, tol, max_steps, out_beta, out_coef, out_intercept, out_decision, out_steps);
    });
}

int pgx_svm_bag_dev(pgx_ctx *ctx, const uint64_t *d_bits, uint32_t n_rows, uint32_t n_genomes, const uint64_t *d_masks,
                    uint32_t n_masks, const int32_t *d_mask_of_problem, const double *d_C, const uint16_t *d_multiplicity,
                    uint32_t n_problems, const uint8_t *d_labels, double tol, uint32_t max_steps, double *d_beta,
                    double *d_coef, double *d_intercept, double *d_decision, uint32_t *d_steps, void *d_workspace,
                    size_t workspace_bytes, void *stream) {
    return guarded(__func__, [&] {
        return svm_run(ctx, d_bits, n_rows, n_genomes, d_masks, n_masks, d_mask_of_problem, d_C, d_multiplicity, n_problems,
                       d_labels, tol, max_steps, d_beta, d_coef, d_intercept, d_decision, d_steps, d_workspace,
                       workspace_bytes, (hipStream_t)stream);
    });
}

}  // extern "C"
