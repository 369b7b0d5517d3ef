// Coordinate descent on the Bernoulli grid likelihood on gfx950 (compute_bernoulli_grid_core_genome_cd), the whole loop
// on the device: DESIGN.md 6g.
//
// Model as in bernoulli.hip: gene i occurs in genome j with probability p_i q_j. One iteration is
//   row sweep     for every gene i, Q fixed:       the root in [lo, hi] of
//                     f(p) = rowsum_i / p - sum_{j absent} q_j / (1 - p q_j)            (= dLL / dp_i)
//   column sweep  for every genome j, the NEW P:   the same with the roles exchanged
//   likelihood    LL at the new (P, Q)
// Jacobi inside a sweep (no solve reads what another solve of its sweep writes), Gauss-Seidel between sweeps.
// Around each root problem stands the rule of the reference: f is taken at both bounds; when f(lo) f(hi) >= 0 the
// solve returns the bound NEARER to the coordinate's previous value (lo when |last - lo| < |last - hi|, strictly,
// else hi) -- an all-present row (f > 0 at both ends) and an all-absent one (f < 0) go there too -- and otherwise the
// root is found by Brent's method (R. P. Brent, Algorithms for Minimization without Derivatives, 1973, ch. 4: a bracket
// [b, c] with the best point b, inverse quadratic or secant steps while they shrink the bracket fast enough, bisection
// otherwise), stopped when half the bracket is below (xtol + rtol |b|) / 2 or f(b) == 0, with xtol = 2e-12,
// rtol = 4 x 2^-52, at most 100 steps (scipy's brentq defaults). A solve that has not stopped by then is counted and
// fails the call.
//
// Log flavour (PGX_BERNOULLI_CD_LOGS): the variables are lp = log p, lq = log q, the bounds log lo, log hi, and
//   f(lp) = rowsum exp(-lp) - sum_{j absent} exp(lq_j) / (-expm1(lp + lq_j))
//   LL    = sum X (lp + lq) + (1 - X) log(-expm1(lp + lq))
// It is the second instantiation of the same kernels. exp(lq_j) is taken once per sweep (ex[]), as the reference's
// numerator is.
//
// Arithmetic: fp64, no contraction (an fma in 1 - p q moves that term by 5e-9 near the upper bound), IEEE division;
// p q, 1 - p q and each quotient are rounded once each. Deterministic: no atomics; every sum's order is fixed by the
// shape alone:
//   row solve     one lane per gene; an evaluation walks the genomes in ascending order and adds the absent cells'
//                 terms one after the other (one bitmap word and one q_j per step, the same address across the wave)
//   column solve  one workgroup of 256 threads per genome; thread t owns the bitmap words t, t + 256, ... and adds
//                 their absent genes' terms in ascending order; the 256 partials are summed in a fixed tree in LDS.
//                 Every thread of the workgroup carries the same Brent state, so the loop is uniform.
// Pad bits beyond n_genes are never cells: a row solve reads its own bit only, the column solve masks the last word.
#include <cmath>
#include <new>

#include "pgx_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr uint32_t CD_ROW_THREADS = 64;      // one wave per workgroup: 40,000 genes are 625 workgroups over 256 CUs
constexpr uint32_t CD_COL_THREADS = 256;
constexpr uint32_t CD_THREADS = 256;
constexpr double CD_XTOL = 2e-12;
constexpr double CD_RTOL = 0x1p-50;          // 4 x 2^-52
constexpr uint32_t CD_MAXITER = 100;
constexpr uint32_t CD_MAX_ITERATIONS = 1u << 20;

struct CdGeom {
    size_t off_par, off_stats, off_pq, off_ex, off_cnt, off_evsum, off_evmax, off_fail, off_terms, off_eval, off_bern;
    size_t bern_bytes, bytes;
};

CdGeom make_geom(uint32_t G, uint32_t S) {
    CdGeom g;
    const size_t n = (size_t)G + S;
    WsLayout ws;
    g.off_par = ws.take(256);                        // the two bounds in the solver's variable
    g.off_stats = ws.take(256);                      // 4 x u64: evaluations, most evaluations of one solve, failures
    g.off_pq = ws.take(n * 8);                       // the solver's variables [P; Q] (or their logs)
    g.off_ex = ws.take(n * 8);                       // log flavour: exp of them
    g.off_cnt = ws.take(n * 4);                      // rowsum, colsum
    g.off_evsum = ws.take(n * 4);
    g.off_evmax = ws.take(n * 4);
    g.off_fail = ws.take(n * 4);
    g.off_terms = ws.take(n * 8);                    // log flavour: each row's and column's share of LL
    g.off_eval = ws.take((n + 1) * 8);               // [LL; gradient] of pgx_bernoulli_eval_dev
    g.bern_bytes = pgx_bernoulli_workspace_bytes(G, S);
    g.off_bern = ws.take(g.bern_bytes);
    g.bytes = ws.off;
    return g;
}

struct CdSolve {
    double x;
    uint32_t evals, failed;
};

// The rule around the solver and Brent's method. f(x) is called at ONE place, so that the lanes of a wave (row solve)
// evaluate together whatever phase each is in, and a workgroup (column solve) meets its barriers together.
template <typename F>
__device__ __forceinline__ CdSolve cd_solve(F &f, double lo, double hi, double last) {
    CdSolve out;
    out.evals = 0;
    out.failed = 0;
    double a = lo, b = hi, c = lo, fa = 0.0, fb = 0.0, fc = 0.0, d = 0.0, e = 0.0;
    double x = lo;
    uint32_t phase = 0, steps = 0;
    bool done = false;
    while (!done) {
        const double fx = f(x);
        ++out.evals;
        if (phase == 0) {                    // f(lo)
            fa = fx;
            x = hi;
            phase = 1;
            continue;
        }
        fb = fx;
        if (phase == 1) {                    // f(hi): the boundary rule, or the first bracket
            phase = 2;
            if (fa * fb >= 0.0) {
                out.x = fabs(last - lo) < fabs(last - hi) ? lo : hi;
                done = true;
                continue;
            }
            c = a;
            fc = fa;
            d = e = b - a;
        }
        if ((fb > 0.0 && fc > 0.0) || (fb < 0.0 && fc < 0.0)) {
            c = a;
            fc = fa;
            d = e = b - a;
        }
        if (fabs(fc) < fabs(fb)) {
            a = b; b = c; c = a;
            fa = fb; fb = fc; fc = fa;
        }
        const double tol1 = (CD_XTOL + CD_RTOL * fabs(b)) / 2.0;
        const double xm = (c - b) / 2.0;
        if (fabs(xm) < tol1 || fb == 0.0) {
            out.x = b;
            done = true;
            continue;
        }
        if (steps == CD_MAXITER) {
            out.x = b;
            out.failed = 1;
            done = true;
            continue;
        }
        ++steps;
        if (fabs(e) >= tol1 && fabs(fa) > fabs(fb)) {
            const double s = fb / fa;
            double p, q;
            if (a == c) {                    // secant
                p = 2.0 * xm * s;
                q = 1.0 - s;
            } else {                         // inverse quadratic interpolation
                const double qq = fa / fc, r = fb / fc;
                p = s * (2.0 * xm * qq * (qq - r) - (b - a) * (r - 1.0));
                q = (qq - 1.0) * (r - 1.0) * (s - 1.0);
            }
            if (p > 0.0) q = -q;
            p = fabs(p);
            if (2.0 * p < fmin(3.0 * xm * q - fabs(tol1 * q), fabs(e * q))) {
                e = d;
                d = p / q;
            } else {
                d = xm;
                e = d;
            }
        } else {
            d = xm;
            e = d;
        }
        a = b;
        fa = fb;
        b += fabs(d) > tol1 ? d : (xm > 0.0 ? tol1 : -tol1);
        x = b;
    }
    return out;
}

// rowsum_i (k < G) and colsum_j (k >= G), once per call
__global__ __launch_bounds__(CD_THREADS) void bcd_count_kernel(const unsigned long long *__restrict__ bits, uint32_t stride,
                                                               uint32_t G, uint32_t S, uint32_t *__restrict__ cnt) {
    const uint32_t k = blockIdx.x * CD_THREADS + threadIdx.x;
    if (k >= G + S) return;
    uint32_t n = 0;
    if (k < G) {
        const uint32_t w = k >> 6, b = k & 63u;
        for (uint32_t j = 0; j < S; ++j) n += (uint32_t)((bits[(size_t)j * stride + w] >> b) & 1ull);
    } else {
        const unsigned long long *row = bits + (size_t)(k - G) * stride;
        const uint32_t words = (G + 63) / 64;
        for (uint32_t w = 0; w < words; ++w) {
            const uint32_t nb = min(64u, G - w * 64);
            const unsigned long long valid = nb == 64 ? ~0ull : ((1ull << nb) - 1ull);
            n += (uint32_t)__popcll(row[w] & valid);
        }
    }
    cnt[k] = n;
}

// the start point in the solver's variable, the bounds in it, and the per-solve counters cleared
template <bool LOGS>
__global__ __launch_bounds__(CD_THREADS) void bcd_init_kernel(const double *__restrict__ init_p, double init_q, double lo,
                                                              double hi, uint32_t G, uint32_t S, double *__restrict__ par,
                                                              double *__restrict__ pq, double *__restrict__ ex,
                                                              uint32_t *__restrict__ evsum, uint32_t *__restrict__ evmax,
                                                              uint32_t *__restrict__ fail) {
    const uint32_t k = blockIdx.x * CD_THREADS + threadIdx.x;
    if (k == 0) {
        par[0] = LOGS ? log(lo) : lo;
        par[1] = LOGS ? log(hi) : hi;
    }
    if (k >= G + S) return;
    const double v = k < G ? init_p[k] : init_q;
    const double x = LOGS ? log(v) : v;
    pq[k] = x;
    ex[k] = LOGS ? exp(x) : x;
    evsum[k] = 0;
    evmax[k] = 0;
    fail[k] = 0;
}

template <bool LOGS>
__global__ __launch_bounds__(CD_ROW_THREADS) void bcd_rows_kernel(const unsigned long long *__restrict__ bits,
                                                                  uint32_t stride, uint32_t G, uint32_t S,
                                                                  const uint32_t *__restrict__ cnt,
                                                                  const double *__restrict__ par, double *pq, double *ex,
                                                                  uint32_t *__restrict__ evsum, uint32_t *__restrict__ evmax,
                                                                  uint32_t *__restrict__ fail) {
    const uint32_t i = blockIdx.x * CD_ROW_THREADS + threadIdx.x;
    if (i >= G) return;
    const unsigned long long *col = bits + (i >> 6);
    const uint32_t b = i & 63u;
    const double *q = pq + G, *eq = ex + G;
    const double n = (double)cnt[i];
    auto f = [&](double x) -> double {
        double s = 0.0;
        for (uint32_t j = 0; j < S; ++j) {
            if ((col[(size_t)j * stride] >> b) & 1ull) continue;
            if (LOGS) {
                s += eq[j] / (-expm1(x + q[j]));
            } else {
                const double qj = q[j];
                const double r = x * qj;
                const double t = 1.0 - r;
                s += qj / t;
            }
        }
        return LOGS ? n * exp(-x) - s : n / x - s;
    };
    const CdSolve r = cd_solve(f, par[0], par[1], pq[i]);
    pq[i] = r.x;
    if (LOGS) ex[i] = exp(r.x);
    evsum[i] += r.evals;
    evmax[i] = max(evmax[i], r.evals);
    fail[i] += r.failed;
}

template <bool LOGS>
__global__ __launch_bounds__(CD_COL_THREADS) void bcd_cols_kernel(const unsigned long long *__restrict__ bits,
                                                                  uint32_t stride, uint32_t G, uint32_t S,
                                                                  const uint32_t *__restrict__ cnt,
                                                                  const double *__restrict__ par, double *pq, double *ex,
                                                                  uint32_t *__restrict__ evsum, uint32_t *__restrict__ evmax,
                                                                  uint32_t *__restrict__ fail) {
    __shared__ double s_part[CD_COL_THREADS];
    const uint32_t j = blockIdx.x, t = threadIdx.x;
    const unsigned long long *row = bits + (size_t)j * stride;
    const uint32_t words = (G + 63) / 64;
    const double n = (double)cnt[G + j];
    auto f = [&](double x) -> double {
        double s = 0.0;
        for (uint32_t w = t; w < words; w += CD_COL_THREADS) {
            const uint32_t base = w * 64;
            const uint32_t nb = min(64u, G - base);                 // pad bits beyond G are not cells
            const unsigned long long valid = nb == 64 ? ~0ull : ((1ull << nb) - 1ull);
            for (unsigned long long z = ~row[w] & valid; z; z &= z - 1ull) {
                const uint32_t i = base + (uint32_t)__builtin_ctzll(z);
                if (LOGS) {
                    s += ex[i] / (-expm1(x + pq[i]));
                } else {
                    const double pi = pq[i];
                    const double r = x * pi;
                    const double u = 1.0 - r;
                    s += pi / u;
                }
            }
        }
        s_part[t] = s;
        __syncthreads();
        for (uint32_t d = CD_COL_THREADS / 2; d > 0; d >>= 1) {
            if (t < d) s_part[t] += s_part[t + d];
            __syncthreads();
        }
        const double sum = s_part[0];
        __syncthreads();
        return LOGS ? n * exp(-x) - sum : n / x - sum;
    };
    const CdSolve r = cd_solve(f, par[0], par[1], pq[G + j]);      // (the same in every thread of the workgroup)
    if (t == 0) {
        pq[G + j] = r.x;
        if (LOGS) ex[G + j] = exp(r.x);
        evsum[G + j] += r.evals;
        evmax[G + j] = max(evmax[G + j], r.evals);
        fail[G + j] += r.failed;
    }
}

// log flavour: row k's share of LL, rowsum lp + sum over its absent cells of log(-expm1(lp + lq)), and column j's colsum lq
__global__ __launch_bounds__(CD_THREADS) void bcd_ll_log_kernel(const unsigned long long *__restrict__ bits, uint32_t stride,
                                                                uint32_t G, uint32_t S, const uint32_t *__restrict__ cnt,
                                                                const double *__restrict__ pq, double *__restrict__ terms) {
    const uint32_t k = blockIdx.x * CD_THREADS + threadIdx.x;
    if (k >= G + S) return;
    const double x = pq[k];
    double s = 0.0;
    if (k < G) {
        const unsigned long long *col = bits + (k >> 6);
        const uint32_t b = k & 63u;
        for (uint32_t j = 0; j < S; ++j)
            if (!((col[(size_t)j * stride] >> b) & 1ull)) s += log(-expm1(x + pq[G + j]));
    }
    const uint32_t n = cnt[k];
    terms[k] = n ? (double)n * x + s : s;
}

__global__ __launch_bounds__(1024) void bcd_total_kernel(const double *__restrict__ terms, uint32_t n,
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

// column `col` of the result tables: row 0 = LL, rows 1.. = the variables (table: their exp in the log flavour)
__global__ __launch_bounds__(CD_THREADS) void bcd_store_kernel(uint32_t n, uint32_t n_cols, uint32_t col, uint32_t logs,
                                                               const double *__restrict__ ll, const double *__restrict__ pq,
                                                               const double *__restrict__ ex, double *__restrict__ table,
                                                               double *__restrict__ solver) {
    const uint32_t k = blockIdx.x * CD_THREADS + threadIdx.x;
    if (k > n) return;
    const size_t o = (size_t)k * n_cols + col;
    const double v = k == 0 ? ll[0] : pq[k - 1];
    table[o] = (k == 0 || !logs) ? v : ex[k - 1];
    if (solver) solver[o] = v;
}

__global__ __launch_bounds__(1024) void bcd_stats_kernel(uint32_t n, const uint32_t *__restrict__ evsum,
                                                         const uint32_t *__restrict__ evmax, const uint32_t *__restrict__ fail,
                                                         unsigned long long *__restrict__ stats) {
    __shared__ unsigned long long s_sum[1024], s_fail[1024];
    __shared__ uint32_t s_max[1024];
    unsigned long long sum = 0, bad = 0;
    uint32_t most = 0;
    for (uint32_t k = threadIdx.x; k < n; k += 1024) {
        sum += evsum[k];
        bad += fail[k];
        most = max(most, evmax[k]);
    }
    s_sum[threadIdx.x] = sum;
    s_fail[threadIdx.x] = bad;
    s_max[threadIdx.x] = most;
    __syncthreads();
    for (uint32_t d = 512; d > 0; d >>= 1) {
        if (threadIdx.x < d) {
            s_sum[threadIdx.x] += s_sum[threadIdx.x + d];
            s_fail[threadIdx.x] += s_fail[threadIdx.x + d];
            s_max[threadIdx.x] = max(s_max[threadIdx.x], s_max[threadIdx.x + d]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        stats[0] = s_sum[0];
        stats[1] = s_max[0];
        stats[2] = s_fail[0];
        stats[3] = 0;
    }
}

int check_arguments(uint32_t G, uint32_t S, double init_q, double lo, double hi, uint32_t n_iterations, uint32_t flags) {
    PGX_REQUIRE(G != 0 && S != 0, "an empty table");
    PGX_REQUIRE((uint64_t)G + S < (1ull << 31), "table too large");
    PGX_REQUIRE((flags & ~(uint32_t)PGX_BERNOULLI_CD_LOGS) == 0, "unknown flag");
    PGX_REQUIRE(n_iterations <= CD_MAX_ITERATIONS, "too many iterations");
    PGX_REQUIRE(std::isfinite(lo) && std::isfinite(hi) && std::isfinite(init_q), "a bound or init_q is not finite");
    PGX_REQUIRE(0.0 < lo && lo < hi, "the bounds must satisfy 0 < lo < hi");
    PGX_REQUIRE(init_q > 0.0, "init_q must be positive");
    PGX_REQUIRE(hi * std::max(hi, init_q) < 1.0, "hi x max(hi, init_q) must stay below 1");
    return PGX_OK;
}

// Everything of one call, enqueued on `stream`; the statistics are left in the workspace.
template <bool LOGS>
int enqueue(pgx_ctx *ctx, const uint64_t *d_bits_, uint32_t G, uint32_t S, const double *d_init_p, double init_q, double lo,
            double hi, uint32_t T, double *d_table, double *d_solver, char *ws, const CdGeom &g, hipStream_t stream) {
    const unsigned long long *d_bits = (const unsigned long long *)d_bits_;
    const uint32_t n = G + S, stride = pgx_bitmap_stride_words(G), n_cols = T + 1;
    double *par = (double *)(ws + g.off_par), *pq = (double *)(ws + g.off_pq), *ex = (double *)(ws + g.off_ex);
    double *terms = (double *)(ws + g.off_terms), *eval = (double *)(ws + g.off_eval);
    uint32_t *cnt = (uint32_t *)(ws + g.off_cnt), *evsum = (uint32_t *)(ws + g.off_evsum);
    uint32_t *evmax = (uint32_t *)(ws + g.off_evmax), *fail = (uint32_t *)(ws + g.off_fail);
    const uint32_t blocks_n = ceil_div_u32(n, CD_THREADS);
    {
        ProfScope prof(ctx, "bcd_count_kernel", stream);
        bcd_count_kernel<<<blocks_n, CD_THREADS, 0, stream>>>(d_bits, stride, G, S, cnt);
    }
    PGX_HIP(hipGetLastError());
    {
        ProfScope prof(ctx, "bcd_init_kernel", stream);
        bcd_init_kernel<LOGS><<<blocks_n, CD_THREADS, 0, stream>>>(d_init_p, init_q, lo, hi, G, S, par, pq, ex, evsum, evmax,
                                                                  fail);
    }
    PGX_HIP(hipGetLastError());
    for (uint32_t it = 0; it <= T; ++it) {
        if (it) {
            {
                ProfScope prof(ctx, LOGS ? "bcd_rows_log_kernel" : "bcd_rows_kernel", stream);
                bcd_rows_kernel<LOGS><<<ceil_div_u32(G, CD_ROW_THREADS), CD_ROW_THREADS, 0, stream>>>(
                    d_bits, stride, G, S, cnt, par, pq, ex, evsum, evmax, fail);
            }
            PGX_HIP(hipGetLastError());
            {
                ProfScope prof(ctx, LOGS ? "bcd_cols_log_kernel" : "bcd_cols_kernel", stream);
                bcd_cols_kernel<LOGS><<<S, CD_COL_THREADS, 0, stream>>>(d_bits, stride, G, S, cnt, par, pq, ex, evsum, evmax,
                                                                        fail);
            }
            PGX_HIP(hipGetLastError());
        }
        if (LOGS) {
            {
                ProfScope prof(ctx, "bcd_ll_log_kernel", stream);
                bcd_ll_log_kernel<<<blocks_n, CD_THREADS, 0, stream>>>(d_bits, stride, G, S, cnt, pq, terms);
            }
            PGX_HIP(hipGetLastError());
            {
                ProfScope prof(ctx, "bcd_total_kernel", stream);
                bcd_total_kernel<<<1, 1024, 0, stream>>>(terms, n, eval);
            }
            PGX_HIP(hipGetLastError());
        } else {   // the kernels of bernoulli.hip, under their accuracy rule (every p q is a normal number below 1)
            const int rc = pgx_bernoulli_eval_dev(ctx, d_bits_, G, S, pq, 0, eval, ws + g.off_bern, g.bern_bytes, stream);
            if (rc != PGX_OK) return rc;
        }
        {
            ProfScope prof(ctx, "bcd_store_kernel", stream);
            bcd_store_kernel<<<ceil_div_u32(n + 1, CD_THREADS), CD_THREADS, 0, stream>>>(n, n_cols, it, LOGS ? 1u : 0u, eval,
                                                                                        pq, ex, d_table, d_solver);
        }
        PGX_HIP(hipGetLastError());
    }
    {
        ProfScope prof(ctx, "bcd_stats_kernel", stream);
        bcd_stats_kernel<<<1, 1024, 0, stream>>>(n, evsum, evmax, fail, (unsigned long long *)(ws + g.off_stats));
    }
    PGX_HIP(hipGetLastError());
    return PGX_OK;
}

int enqueue_any(pgx_ctx *ctx, const uint64_t *d_bits, uint32_t G, uint32_t S, const double *d_init_p, double init_q, double lo,
                double hi, uint32_t T, uint32_t flags, double *d_table, double *d_solver, char *ws, const CdGeom &g,
                hipStream_t stream) {
    return (flags & PGX_BERNOULLI_CD_LOGS)
               ? enqueue<true>(ctx, d_bits, G, S, d_init_p, init_q, lo, hi, T, d_table, d_solver, ws, g, stream)
               : enqueue<false>(ctx, d_bits, G, S, d_init_p, init_q, lo, hi, T, d_table, d_solver, ws, g, stream);
}

// after the stream has been synchronised
int read_statistics(pgx_ctx *ctx, uint32_t G, uint32_t S, uint32_t T) {
    ctx->bern_cd_stats[3] = (uint64_t)((uint64_t)G + S) * T;
    if (ctx->bern_cd_stats[2] != 0) {
        pgx_set_error("pgx_bernoulli_cd: %llu of %llu solves did not converge in %u steps",
                      (unsigned long long)ctx->bern_cd_stats[2], (unsigned long long)ctx->bern_cd_stats[3], CD_MAXITER);
        return PGX_ERR_INTERNAL;
    }
    return PGX_OK;
}

int cd_dev(pgx_ctx *ctx, const uint64_t *d_bits, uint32_t G, uint32_t S, const double *d_init_p, double init_q, double lo,
           double hi, uint32_t T, uint32_t flags, double *d_table, double *d_solver, void *d_ws, size_t ws_bytes,
           void *stream_) {
    PGX_REQUIRE(ctx, "NULL context");
    int rc = check_arguments(G, S, init_q, lo, hi, T, flags);
    if (rc != PGX_OK) return rc;
    PGX_REQUIRE(d_bits && d_init_p && d_table && d_ws, "NULL argument");
    const CdGeom g = make_geom(G, S);
    PGX_REQUIRE(ws_bytes >= g.bytes, "workspace too small (see pgx_bernoulli_cd_workspace_bytes)");
    hipStream_t stream = (hipStream_t)stream_;
    rc = enqueue_any(ctx, d_bits, G, S, d_init_p, init_q, lo, hi, T, flags, d_table, d_solver, (char *)d_ws, g, stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(hipMemcpyAsync(ctx->bern_cd_stats, (char *)d_ws + g.off_stats, 32, hipMemcpyDeviceToHost, stream));
    PGX_HIP(hipStreamSynchronize(stream));
    return read_statistics(ctx, G, S, T);
}

int cd_loaded(pgx_ctx *ctx, const double *init_p, double init_q, double lo, double hi, uint32_t T, uint32_t flags,
              double *out_table, double *out_solver) {
    PGX_REQUIRE(ctx && init_p && out_table, "NULL argument");
    PGX_REQUIRE(ctx->bern_loaded, "no table loaded (pgx_bernoulli_load / pgx_bernoulli_load_resident)");
    const uint32_t G = ctx->bern_genes, S = ctx->bern_genomes;
    int rc = check_arguments(G, S, init_q, lo, hi, T, flags);
    if (rc != PGX_OK) return rc;
    for (uint32_t i = 0; i < G; ++i)
        PGX_REQUIRE(init_p[i] >= lo && init_p[i] <= hi, "init_p must lie inside the bounds (clip it)");
    PGX_HIP(hipSetDevice(ctx->device_id));
    const CdGeom g = make_geom(G, S);
    const size_t cells = ((size_t)G + S + 1) * ((size_t)T + 1);
    DevBuf d_bits(ctx, PGX_SLOT_BERN_BITS), d_init(ctx, CD_SLOT_INIT), d_table(ctx, CD_SLOT_TABLE);
    DevBuf d_solver(ctx, CD_SLOT_SOLVER), d_ws(ctx, CD_SLOT_WS);
    rc = d_bits.view((size_t)S * pgx_bitmap_stride_words(G) * 8);        // (the loaded table)
    if (rc != PGX_OK) return rc;
    PGX_HIP(d_init.alloc((size_t)G * 8));
    PGX_HIP(d_table.alloc(cells * 8));
    if (out_solver) PGX_HIP(d_solver.alloc(cells * 8));
    PGX_HIP(d_ws.alloc(g.bytes));
    PGX_HIP(hipMemcpyAsync(d_init.p, init_p, (size_t)G * 8, hipMemcpyHostToDevice, ctx->stream));
    rc = enqueue_any(ctx, d_bits.as<uint64_t>(), G, S, d_init.as<double>(), init_q, lo, hi, T, flags, d_table.as<double>(),
                     out_solver ? d_solver.as<double>() : nullptr, (char *)d_ws.p, g, ctx->stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(hipMemcpyAsync(out_table, d_table.p, cells * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (out_solver) PGX_HIP(hipMemcpyAsync(out_solver, d_solver.p, cells * 8, hipMemcpyDeviceToHost, ctx->stream));
    PGX_HIP(hipMemcpyAsync(ctx->bern_cd_stats, (char *)d_ws.p + g.off_stats, 32, hipMemcpyDeviceToHost, ctx->stream));
    PGX_HIP(hipStreamSynchronize(ctx->stream));
    return read_statistics(ctx, G, S, T);
}

int copy_statistics(pgx_ctx *ctx, uint64_t *out_stats) {
    PGX_REQUIRE(ctx && out_stats, "NULL argument");
    for (int k = 0; k < 4; ++k) out_stats[k] = ctx->bern_cd_stats[k];
    return PGX_OK;
}

}  // namespace

extern "C" {

size_t pgx_bernoulli_cd_workspace_bytes(uint32_t n_genes, uint32_t n_genomes) {
    try {
        return make_geom(n_genes, n_genomes).bytes;
    } catch (...) {
        return 0;
    }
}

int pgx_bernoulli_cd_dev(pgx_ctx *ctx, const uint64_t *d_bits, uint32_t n_genes, uint32_t n_genomes, const double *d_init_p,
                         double init_q, double lo, double hi, uint32_t n_iterations, uint32_t flags, double *d_out_table,
                         double *d_out_solver_table, void *d_workspace, size_t workspace_bytes, void *stream) {
    return guarded(__func__, [&] {
        return cd_dev(ctx, d_bits, n_genes, n_genomes, d_init_p, init_q, lo, hi, n_iterations, flags, d_out_table,
                      d_out_solver_table, d_workspace, workspace_bytes, stream);
    });
}

int pgx_bernoulli_cd(pgx_ctx *ctx, const double *init_p, double init_q, double lo, double hi, uint32_t n_iterations,
                     uint32_t flags, double *out_table, double *out_solver_table) {
    return guarded(__func__, [&] {
        return cd_loaded(ctx, init_p, init_q, lo, hi, n_iterations, flags, out_table, out_solver_table);
    });
}

int pgx_bernoulli_cd_stats(pgx_ctx *ctx, uint64_t *out_stats) {
    return guarded(__func__, [&] { return copy_statistics(ctx, out_stats); });
}

}  // extern "C"
