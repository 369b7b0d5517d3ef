// Monte-Carlo Kolmogorov-Smirnov test of a beta-binomial fit on gfx950 (ks_montecarlo_bbn / draw_bbn of
// compute_beta_binomial_core_genome).
//
// The reference draws n_samples x iterations values with np.random.choice(arange(L), p=probs) on numpy's legacy
// generator and, per iteration, builds the eCDF with np.unique and a Python loop. Here:
//   host    the generator: MT19937 twist + tempering (pgx_legacy_uniform_words, ingest.cpp), chunk by chunk into
//           page-locked staging buffers; two buffers, so the twist of chunk k+1 overlaps the copy and kernel of chunk k
//   device  everything after the words (bbn_ks_kernel): per iteration, the draws' doubles, searchsorted(side='right')
//           over the normalised cdf, an integer histogram, its prefix sum, the fp64 eCDF and the max distance to the
//           model cdf. One workgroup per iteration, a workgroup looping over iterations when there are more of them
//           than workgroups (so the cdf is loaded into LDS once per workgroup, not per iteration).
// Bit-identity with the reference: the double of a draw is exact arithmetic on the two words; the search returns the
// reference's index for any non-decreasing cdf; the histogram and its prefix sums are integers (exact, whatever the
// order of the atomics); cumsum / n_samples is one rounded division, as numpy's float64 cumsum of integer counts
// divided by their (exact) sum; the max of exact values does not depend on the order. nan propagates as in np.max.
//
// Up to PGX_BBN_LDS_LIMIT values the cdf (8 B) and the histogram (4 B) of a workgroup live in LDS (48 KiB at the
// limit); above it both stay in global memory: the cdf read through the caches, one histogram per workgroup in the
// caller's workspace.
#include <new>

#include "pgx_internal.h"

namespace {

constexpr uint32_t BB_THREADS = 256;
constexpr uint32_t BB_WAVES = BB_THREADS / 64;
constexpr uint32_t BB_MAX_BLOCKS = 1024;            // 256 CUs x 4 workgroups
constexpr uint64_t BB_CHUNK_DRAWS = 1ull << 22;     // default: 32 MiB of words per chunk
constexpr uint32_t BB_LDS_LIMIT = PGX_BBN_LDS_LIMIT;

// numpy's legacy random_sample(): ((w0 >> 5) * 2^26 + (w1 >> 6)) / 2^53, every step exact
__device__ __forceinline__ double legacy_double(uint2 w) {
    const double a = (double)(w.x >> 5), b = (double)(w.y >> 6);
    return (a * 67108864.0 + b) / 9007199254740992.0;
}

// searchsorted(cdf, u, side='right'): the number of entries <= u (cdf non-decreasing, no nan)
__device__ __forceinline__ uint32_t search_right(const double *cdf, uint32_t L, double u) {
    uint32_t lo = 0, hi = L;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (cdf[mid] <= u) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// np.max's rule: a nan anywhere is the result
__device__ __forceinline__ double nan_max(double m, double d) { return (d > m || d != d) ? d : m; }

template <bool kLds>
__device__ __forceinline__ uint32_t hist_load(const uint32_t *h) {
    if constexpr (kLds) return *h;
    // (the global histogram is built by atomics at L2: read it there, not from a possibly stale L1 line)
    else return __hip_atomic_load(h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool kLds>
__global__ __launch_bounds__(BB_THREADS) void bbn_ks_kernel(const uint2 *__restrict__ draws, const double *__restrict__ draw_cdf,
                                                            const double *__restrict__ model_cdf, uint32_t L,
                                                            uint32_t n_samples, uint32_t iterations,
                                                            uint32_t *__restrict__ g_hist, double *__restrict__ ks_sim) {
    extern __shared__ double lds_cdf[];                 // kLds: cdf[L], then hist[L]
    __shared__ uint32_t s_part[BB_THREADS];
    __shared__ double s_wmax[BB_WAVES];
    const uint32_t t = threadIdx.x;
    const double *cdf = draw_cdf;
    uint32_t *hist = g_hist + (size_t)blockIdx.x * L;
    if constexpr (kLds) {
        for (uint32_t j = t; j < L; j += BB_THREADS) lds_cdf[j] = draw_cdf[j];
        cdf = lds_cdf;
        hist = reinterpret_cast<uint32_t *>(lds_cdf + L);
    }
    // thread t owns the values [j0, j1) of the prefix sum
    const uint32_t seg = (L + BB_THREADS - 1) / BB_THREADS;
    const uint32_t j0 = min(L, t * seg), j1 = min(L, j0 + seg);
    const double n = (double)n_samples;
    for (uint32_t it = blockIdx.x; it < iterations; it += gridDim.x) {
        for (uint32_t j = t; j < L; j += BB_THREADS) hist[j] = 0;
        __syncthreads();
        const uint2 *w = draws + (uint64_t)it * n_samples;
        for (uint32_t d = t; d < n_samples; d += BB_THREADS) {
            const uint32_t k = search_right(cdf, L, legacy_double(w[d]));
            if (k < L) atomicAdd(&hist[k], 1u);         // (k == L needs u >= cdf[L-1] = 1: never; kept in bounds)
        }
        __syncthreads();
        uint32_t local = 0;
        for (uint32_t j = j0; j < j1; ++j) local += hist_load<kLds>(&hist[j]);
        s_part[t] = local;
        __syncthreads();
        for (uint32_t off = 1; off < BB_THREADS; off <<= 1) {      // inclusive scan of the 256 segment sums
            const uint32_t v = t >= off ? s_part[t - off] : 0u;
            __syncthreads();
            s_part[t] += v;
            __syncthreads();
        }
        uint32_t cum = s_part[t] - local;
        double m = -INFINITY;
        for (uint32_t j = j0; j < j1; ++j) {
            cum += hist_load<kLds>(&hist[j]);
            m = nan_max(m, fabs((double)cum / n - model_cdf[j]));
        }
        for (int off = 32; off > 0; off >>= 1) m = nan_max(m, __shfl_xor(m, off, 64));
        if ((t & 63) == 0) s_wmax[t >> 6] = m;
        __syncthreads();
        if (t == 0) {
            double r = s_wmax[0];
            for (uint32_t k = 1; k < BB_WAVES; ++k) r = nan_max(r, s_wmax[k]);
            ks_sim[it] = r;
        }
    }
}

template <bool kLds>
__global__ __launch_bounds__(BB_THREADS) void bbn_draws_kernel(const uint2 *__restrict__ draws, const double *__restrict__ draw_cdf,
                                                               uint32_t L, uint64_t n, int64_t *__restrict__ out) {
    extern __shared__ double lds_cdf[];
    const double *cdf = draw_cdf;
    if constexpr (kLds) {
        for (uint32_t j = threadIdx.x; j < L; j += BB_THREADS) lds_cdf[j] = draw_cdf[j];
        __syncthreads();
        cdf = lds_cdf;
    }
    for (uint64_t d = (uint64_t)blockIdx.x * BB_THREADS + threadIdx.x; d < n; d += (uint64_t)gridDim.x * BB_THREADS)
        out[d] = (int64_t)search_right(cdf, L, legacy_double(draws[d]));
}

size_t workspace_bytes(uint32_t L, uint32_t iterations) {
    if (L <= BB_LDS_LIMIT || iterations == 0) return 0;
    return (size_t)std::min(iterations, BB_MAX_BLOCKS) * L * 4;
}

int ks_dev(pgx_ctx *ctx, const uint32_t *d_words, const double *d_draw_cdf, const double *d_model_cdf, uint32_t L,
           uint32_t n_samples, uint32_t iterations, double *d_ks, void *d_ws, size_t ws_bytes, hipStream_t stream) {
    PGX_REQUIRE(ctx && L >= 1 && n_samples >= 1, "sim_limit and n_samples must be at least 1");
    if (iterations == 0) return PGX_OK;
    PGX_REQUIRE(d_words && d_draw_cdf && d_model_cdf && d_ks, "NULL device pointer");
    const size_t need = workspace_bytes(L, iterations);
    PGX_REQUIRE(ws_bytes >= need && (need == 0 || d_ws), "workspace smaller than pgx_bbn_workspace_bytes()");
    const uint32_t grid = std::min(iterations, BB_MAX_BLOCKS);
    const uint2 *words = reinterpret_cast<const uint2 *>(d_words);
    ProfScope prof(ctx, "bbn_ks_kernel", stream);
    if (L <= BB_LDS_LIMIT)
        bbn_ks_kernel<true><<<grid, BB_THREADS, (size_t)L * 12, stream>>>(words, d_draw_cdf, d_model_cdf, L, n_samples,
                                                                         iterations, nullptr, d_ks);
    else
        bbn_ks_kernel<false><<<grid, BB_THREADS, 0, stream>>>(words, d_draw_cdf, d_model_cdf, L, n_samples, iterations,
                                                              static_cast<uint32_t *>(d_ws), d_ks);
    PGX_HIP(hipGetLastError());
    return PGX_OK;
}

struct Events {
    hipEvent_t e[2] = {nullptr, nullptr};
    ~Events() {
        for (auto x : e) if (x) (void)hipEventDestroy(x);
    }
};

uint64_t chunk_of(uint64_t chunk_draws) { return chunk_draws ? chunk_draws : BB_CHUNK_DRAWS; }

int ks_host(pgx_ctx *ctx, const double *draw_cdf, const double *model_cdf, uint32_t L, uint32_t n_samples,
            uint32_t iterations, uint32_t *key, int32_t *pos, uint64_t chunk_draws, double *out) {
    PGX_REQUIRE(ctx && L >= 1 && n_samples >= 1, "sim_limit and n_samples must be at least 1");
    PGX_REQUIRE(key && pos && *pos >= 0 && *pos <= 624, "invalid generator state");
    if (iterations == 0) return PGX_OK;
    PGX_REQUIRE(draw_cdf && model_cdf && out, "NULL argument");
    PGX_HIP(hipSetDevice(ctx->device_id));
    hipStream_t stream = ctx->stream;
    // a chunk: whole iterations, about chunk_draws draws
    const uint32_t per_chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(iterations, chunk_of(chunk_draws) / n_samples));
    const uint64_t chunk_words = 2ull * n_samples * per_chunk;
    HostVec<uint32_t> h0(ctx, BB_HOST_WORDS0, chunk_words), h1(ctx, BB_HOST_WORDS1, chunk_words);
    PGX_REQUIRE(h0.ok() && h1.ok(), "cannot allocate page-locked staging buffers");
    uint32_t *hw[2] = {h0.data(), h1.data()};
    DevBuf dw0(ctx, BB_SLOT_WORDS0), dw1(ctx, BB_SLOT_WORDS1), d_cdf(ctx, BB_SLOT_CDF), d_model(ctx, BB_SLOT_MODEL),
        d_ks(ctx, BB_SLOT_KS), d_hist(ctx, BB_SLOT_HIST);
    const size_t ws = workspace_bytes(L, per_chunk);
    PGX_HIP(dw0.alloc(chunk_words * 4));
    PGX_HIP(dw1.alloc(chunk_words * 4));
    PGX_HIP(d_cdf.alloc((size_t)L * 8));
    PGX_HIP(d_model.alloc((size_t)L * 8));
    PGX_HIP(d_ks.alloc((size_t)iterations * 8));
    PGX_HIP(d_hist.alloc(ws));
    uint32_t *dw[2] = {dw0.as<uint32_t>(), dw1.as<uint32_t>()};
    PGX_HIP(hipMemcpyAsync(d_cdf.p, draw_cdf, (size_t)L * 8, hipMemcpyHostToDevice, stream));
    PGX_HIP(hipMemcpyAsync(d_model.p, model_cdf, (size_t)L * 8, hipMemcpyHostToDevice, stream));
    Events ev;
    for (auto &e : ev.e) PGX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    uint32_t c = 0;
    for (uint32_t it0 = 0; it0 < iterations; it0 += per_chunk, ++c) {
        const uint32_t ni = std::min(per_chunk, iterations - it0);
        const uint64_t words = 2ull * n_samples * ni;
        const int b = c & 1;
        if (c >= 2) PGX_HIP(hipEventSynchronize(ev.e[b]));       // the copy out of this staging buffer is done
        const int rc = pgx_legacy_uniform_words(key, pos, words, hw[b]);
        if (rc != PGX_OK) return rc;
        // (the copy into dw[b] follows the kernel of chunk c-2 that read it: one in-order stream)
        PGX_HIP(hipMemcpyAsync(dw[b], hw[b], words * 4, hipMemcpyHostToDevice, stream));
        PGX_HIP(hipEventRecord(ev.e[b], stream));
        const int rk = ks_dev(ctx, dw[b], d_cdf.as<double>(), d_model.as<double>(), L, n_samples, ni,
                              d_ks.as<double>() + it0, d_hist.p, ws, stream);
        if (rk != PGX_OK) return rk;
    }
    PGX_HIP(hipMemcpyAsync(out, d_ks.p, (size_t)iterations * 8, hipMemcpyDeviceToHost, stream));
    PGX_HIP(hipStreamSynchronize(stream));
    return PGX_OK;
}

int draws_host(pgx_ctx *ctx, const double *draw_cdf, uint32_t L, uint64_t size, uint32_t *key, int32_t *pos,
               uint64_t chunk_draws, int64_t *out) {
    PGX_REQUIRE(ctx && L >= 1, "sim_limit must be at least 1");
    PGX_REQUIRE(key && pos && *pos >= 0 && *pos <= 624, "invalid generator state");
    if (size == 0) return PGX_OK;
    PGX_REQUIRE(draw_cdf && out, "NULL argument");
    PGX_HIP(hipSetDevice(ctx->device_id));
    hipStream_t stream = ctx->stream;
    const uint64_t per_chunk = std::min(size, chunk_of(chunk_draws));
    HostVec<uint32_t> hw(ctx, BB_HOST_WORDS0, 2 * per_chunk);
    HostVec<int64_t> hidx(ctx, BB_HOST_IDX, per_chunk);
    PGX_REQUIRE(hw.ok() && hidx.ok(), "cannot allocate page-locked staging buffers");
    DevBuf dw(ctx, BB_SLOT_WORDS0), d_cdf(ctx, BB_SLOT_CDF), d_idx(ctx, BB_SLOT_IDX);
    PGX_HIP(dw.alloc(per_chunk * 8));
    PGX_HIP(d_cdf.alloc((size_t)L * 8));
    PGX_HIP(d_idx.alloc(per_chunk * 8));
    PGX_HIP(hipMemcpyAsync(d_cdf.p, draw_cdf, (size_t)L * 8, hipMemcpyHostToDevice, stream));
    for (uint64_t done = 0; done < size; done += per_chunk) {
        const uint64_t nd = std::min(per_chunk, size - done);
        const int rc = pgx_legacy_uniform_words(key, pos, 2 * nd, hw.data());
        if (rc != PGX_OK) return rc;
        PGX_HIP(hipMemcpyAsync(dw.p, hw.data(), nd * 8, hipMemcpyHostToDevice, stream));
        const uint32_t grid = (uint32_t)std::min<uint64_t>((nd + BB_THREADS - 1) / BB_THREADS, BB_MAX_BLOCKS);
        {
            ProfScope prof(ctx, "bbn_draws_kernel", stream);
            const uint2 *words = dw.as<const uint2>();
            if (L <= BB_LDS_LIMIT)
                bbn_draws_kernel<true><<<grid, BB_THREADS, (size_t)L * 8, stream>>>(words, d_cdf.as<double>(), L, nd,
                                                                                   d_idx.as<int64_t>());
            else
                bbn_draws_kernel<false><<<grid, BB_THREADS, 0, stream>>>(words, d_cdf.as<double>(), L, nd,
                                                                         d_idx.as<int64_t>());
        }
        PGX_HIP(hipGetLastError());
        PGX_HIP(hipMemcpyAsync(hidx.data(), d_idx.p, nd * 8, hipMemcpyDeviceToHost, stream));
        PGX_HIP(hipStreamSynchronize(stream));
        std::memcpy(out + done, hidx.data(), nd * 8);
    }
    return PGX_OK;
}

}  // namespace

extern "C" {

size_t pgx_bbn_workspace_bytes(uint32_t sim_limit, uint32_t iterations) { return workspace_bytes(sim_limit, iterations); }

int pgx_bbn_ks_sim_dev(pgx_ctx *ctx, const uint32_t *d_words, const double *d_draw_cdf, const double *d_model_cdf,
                       uint32_t sim_limit, uint32_t n_samples, uint32_t iterations, double *d_ks_sim, void *d_workspace,
                       size_t workspace_bytes, void *stream) {
    return guarded(__func__, [&] {
        return ks_dev(ctx, d_words, d_draw_cdf, d_model_cdf, sim_limit, n_samples, iterations, d_ks_sim, d_workspace,
                      workspace_bytes, static_cast<hipStream_t>(stream));
    });
}

int pgx_bbn_ks_sim(pgx_ctx *ctx, const double *draw_cdf, const double *model_cdf, uint32_t sim_limit, uint32_t n_samples,
                   uint32_t iterations, uint32_t *mt_key, int32_t *mt_pos, uint64_t chunk_draws, double *out_ks_sim) {
    return guarded(__func__, [&] {
        return ks_host(ctx, draw_cdf, model_cdf, sim_limit, n_samples, iterations, mt_key, mt_pos, chunk_draws, out_ks_sim);
    });
}

int pgx_bbn_draws(pgx_ctx *ctx, const double *draw_cdf, uint32_t sim_limit, uint64_t size, uint32_t *mt_key,
                  int32_t *mt_pos, uint64_t chunk_draws, int64_t *out_idx) {
    return guarded(__func__, [&] { return draws_host(ctx, draw_cdf, sim_limit, size, mt_key, mt_pos, chunk_draws, out_idx); });
}

}  // extern "C"
