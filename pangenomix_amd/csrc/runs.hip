// Runs of allele rows on the genome-major bitmap (reference pangenome.py:1246-1330 validate_gene_table /
// validate_gene_table_dense and :1812-1889 extract_dominant_alleles): the allele rows of one gene are a contiguous run
// [run_start[r], run_start[r + 1]) of the allele table, and per run
//   derived bit (r, j)  = genome j has any allele bit in run r                  ("gene row = OR of its allele rows")
//   diff                = derived XOR bit gene_of_run[r] of the gene table      (-1: no gene row, the gene bit is 0)
//   total / best        = sum, first maximum and its position of the rows' occupancy counts
// all of it integer work on words the bitmap already holds.
//
// Kernels (plain launches on one stream, no atomics, no workgroup waits for another; every result is independent of the
// order in which the waves run):
//   runs_or_kernel        one lane per run, so a wave is 64 consecutive runs = ONE output word; blockIdx.y takes a slab of
//                         RN_SLAB genomes (run bounds and gene rows are loaded once per slab). A lane masks the first and
//                         the last word of its range and ORs the words between: neighbouring lanes read the same or the
//                         next word. __ballot(any) is the derived word, __ballot(gene bit) the gathered gene word; lane 0
//                         stores both words. Bits of the allele bitmap at or beyond n_alleles are never read unmasked, and
//                         lanes beyond n_runs ballot 0, so the pad bits of the outputs are 0 (their pad WORDS are zeroed by
//                         a memset before the launch).
//   row_counts_kernel     (pancore.hip, through pgx_row_counts_dev) twice: the allele rows' counts, and the popcount of
//                         every row of the diff bitmap = diff_per_run
//   runs_genome_kernel    one workgroup per genome: popcount of its words of the diff bitmap = diff_per_genome
//   runs_stats_kernel     one lane per run over the counts: total (uint64), the first row with the largest count (a
//                         strictly greater count replaces the current one) and that count; an empty run gives 0, -1, 0
//   runs_check_kernel     the device-pointer entry cannot read the caller's run arrays before it launches: this kernel
//                         raises a status bit for a decreasing run_start, an end beyond n_alleles or a gene row out of
//                         range, and every other kernel clamps what it reads, so that bad arrays never become a bad address
#include "pgx_internal.h"

namespace {

constexpr int RN_THREADS = 256;
constexpr uint32_t RN_SLAB = 8;               // genomes per workgroup of runs_or_kernel
constexpr uint32_t RN_ERR_ORDER = 1u, RN_ERR_END = 2u, RN_ERR_GENE = 4u;

struct RunsGeom {
    uint32_t a_stride, o_stride;
    size_t off_diff, off_counts, off_status, bytes;
};

RunsGeom make_geom(uint32_t n_alleles, uint32_t n_runs, uint32_t n_genomes) {
    RunsGeom g;
    g.a_stride = pgx_bitmap_stride_words(n_alleles);
    g.o_stride = pgx_bitmap_stride_words(n_runs);
    WsLayout ws;
    g.off_diff = ws.take((size_t)n_genomes * g.o_stride * 8);
    g.off_counts = ws.take((size_t)n_alleles * 4);
    g.off_status = ws.take(16);
    g.bytes = ws.off;
    return g;
}

bool sizes_ok(uint32_t n_alleles, uint32_t n_runs, uint32_t n_genomes, uint32_t n_genes) {
    return n_alleles < (1u << 31) && n_runs < (1u << 31) && n_genomes < (1u << 31) && n_genes < (1u << 31);
}

__global__ __launch_bounds__(RN_THREADS) void runs_check_kernel(const uint32_t *__restrict__ run_start,
                                                                const int32_t *__restrict__ gene_of_run, uint32_t n_runs,
                                                                uint32_t n_alleles, uint32_t n_genes,
                                                                uint32_t *__restrict__ status) {
    const uint32_t r = blockIdx.x * RN_THREADS + threadIdx.x;
    if (r >= n_runs) return;
    uint32_t bad = 0;
    if (r == 0 && run_start[0] != 0u) bad |= RN_ERR_ORDER;
    if (run_start[r] > run_start[r + 1]) bad |= RN_ERR_ORDER;
    if (run_start[r + 1] > n_alleles) bad |= RN_ERR_END;
    if (gene_of_run && (gene_of_run[r] < -1 || (gene_of_run[r] >= 0 && (uint32_t)gene_of_run[r] >= n_genes))) bad |= RN_ERR_GENE;
    if (bad) atomicOr(status, bad);
}

// derived[j][w] / diff[j][w] for the word w = the wave's 64 runs and the genomes of the workgroup's slabs. Whole waves:
// every lane ballots (the grid covers ceil(n_runs / 64) words exactly, in whole workgroups).
__global__ __launch_bounds__(RN_THREADS) void runs_or_kernel(const unsigned long long *__restrict__ abits, uint32_t a_stride,
                                                             uint32_t n_alleles, const uint32_t *__restrict__ run_start,
                                                             uint32_t n_runs, const unsigned long long *__restrict__ gbits,
                                                             uint32_t g_stride, uint32_t n_genes,
                                                             const int32_t *__restrict__ gene_of_run, uint32_t n_genomes,
                                                             uint32_t o_stride, unsigned long long *__restrict__ derived,
                                                             unsigned long long *__restrict__ diff) {
    const uint32_t r = blockIdx.x * RN_THREADS + threadIdx.x;
    const uint32_t out_word = r >> 6;
    uint32_t s = 0, e = 0, gene = 0xFFFFFFFFu;
    if (r < n_runs) {
        s = min(run_start[r], n_alleles);
        e = min(run_start[r + 1], n_alleles);
        if (gbits && gene_of_run) gene = (uint32_t)gene_of_run[r];      // (-1 and anything out of range: no gene row)
    }
    const bool some = s < e, has_gene = gene < n_genes;
    const uint32_t w0 = s >> 6, w1 = some ? (e - 1u) >> 6 : 0u;         // first and last word of the run (w1 < a_stride)
    const unsigned long long first_mask = ~0ull << (s & 63u);
    const unsigned long long last_mask = ~0ull >> (63u - ((e - 1u) & 63u));
    const bool writer = (threadIdx.x & 63u) == 0 && out_word < o_stride;
    for (uint32_t slab = blockIdx.y; (uint64_t)slab * RN_SLAB < n_genomes; slab += gridDim.y) {
        const uint32_t j0 = slab * RN_SLAB, j1 = min(n_genomes, j0 + RN_SLAB);
        for (uint32_t j = j0; j < j1; ++j) {
            unsigned long long any = 0;
            if (some) {
                const unsigned long long *row = abits + (size_t)j * a_stride;
                for (uint32_t w = w0; w <= w1; ++w) {
                    unsigned long long word = row[w];
                    if (w == w0) word &= first_mask;
                    if (w == w1) word &= last_mask;
                    any |= word;
                }
            }
            const unsigned long long have = __ballot(any != 0ull);
            const unsigned long long want =
                __ballot(has_gene && ((gbits[(size_t)j * g_stride + (gene >> 6)] >> (gene & 63u)) & 1ull) != 0ull);
            if (writer) {
                if (derived) derived[(size_t)j * o_stride + out_word] = have;
                if (diff) diff[(size_t)j * o_stride + out_word] = have ^ want;
            }
        }
    }
}

// out[j] = set bits of the `stride` words of genome j
__global__ __launch_bounds__(RN_THREADS) void runs_genome_kernel(const unsigned long long *__restrict__ bits, uint32_t stride,
                                                                 uint32_t *__restrict__ out) {
    __shared__ uint32_t part[RN_THREADS / 64];
    const unsigned long long *row = bits + (size_t)blockIdx.x * stride;
    uint32_t c = 0;
    for (uint32_t w = threadIdx.x; w < stride; w += RN_THREADS) c += (uint32_t)__popcll(row[w]);
    for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int i = 0; i < RN_THREADS / 64; ++i) t += part[i];
        out[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(RN_THREADS) void runs_stats_kernel(const int32_t *__restrict__ counts, uint32_t n_alleles,
                                                                const uint32_t *__restrict__ run_start, uint32_t n_runs,
                                                                unsigned long long *__restrict__ total,
                                                                int32_t *__restrict__ best_allele,
                                                                uint32_t *__restrict__ best_count) {
    const uint32_t r = blockIdx.x * RN_THREADS + threadIdx.x;
    if (r >= n_runs) return;
    const uint32_t s = min(run_start[r], n_alleles), e = min(run_start[r + 1], n_alleles);
    unsigned long long sum = 0;
    int32_t best = -1;
    uint32_t top = 0;
    for (uint32_t i = s; i < e; ++i) {
        const uint32_t c = (uint32_t)counts[i];
        sum += c;
        if (best < 0 || c > top) { best = (int32_t)i; top = c; }
    }
    if (total) total[r] = sum;
    if (best_allele) best_allele[r] = best;
    if (best_count) best_count[r] = top;
}

}  // namespace

// ---- what select.hip shares with this file (pgx_internal.h) ----
const char *pgx_runs_host_error(const uint32_t *run_start, uint32_t n_runs, const int32_t *gene_of_run, uint32_t n_alleles,
                                uint32_t n_genes) {
    if (n_runs && run_start[0] != 0) return "run_start must start at 0 and never decrease";
    for (uint32_t r = 0; r < n_runs; ++r) {
        if (run_start[r] > run_start[r + 1]) return "run_start must start at 0 and never decrease";
        if (gene_of_run && !(gene_of_run[r] >= -1 && (gene_of_run[r] < 0 || (uint32_t)gene_of_run[r] < n_genes)))
            return "gene_of_run entry out of range";
    }
    if (n_runs && run_start[n_runs] > n_alleles) return "run_start ends beyond the allele rows";
    return nullptr;
}

const char *pgx_runs_status_error(uint32_t status) {
    if (status & RN_ERR_ORDER) return "run_start must start at 0 and never decrease";
    if (status & RN_ERR_END) return "run_start ends beyond the allele rows";
    if (status & RN_ERR_GENE) return "gene_of_run entry out of range";
    return nullptr;
}

int pgx_runs_check_enqueue(pgx_ctx *ctx, const uint32_t *d_run_start, const int32_t *d_gene_of_run, uint32_t n_runs,
                           uint32_t n_alleles, uint32_t n_genes, uint32_t *d_status, hipStream_t stream) {
    {
        ProfScope prof(ctx, "runs_check_kernel", stream);
        runs_check_kernel<<<ceil_div_u32(n_runs, RN_THREADS), RN_THREADS, 0, stream>>>(d_run_start, d_gene_of_run, n_runs,
                                                                                      n_alleles, n_genes, d_status);
    }
    PGX_HIP(hipGetLastError());
    return PGX_OK;
}

int pgx_runs_stats_enqueue(pgx_ctx *ctx, const uint64_t *d_abits, uint32_t n_alleles, uint32_t n_genomes,
                           const uint32_t *d_run_start, uint32_t n_runs, int32_t *d_counts, uint64_t *d_total,
                           int32_t *d_best_allele, uint32_t *d_best_count, hipStream_t stream) {
    const int rc = pgx_row_counts_dev(ctx, d_abits, n_alleles, n_genomes, d_counts, stream);
    if (rc != PGX_OK) return rc;
    ProfScope prof(ctx, "runs_stats_kernel", stream);
    runs_stats_kernel<<<ceil_div_u32(n_runs, RN_THREADS), RN_THREADS, 0, stream>>>(
        d_counts, n_alleles, d_run_start, n_runs, (unsigned long long *)d_total, d_best_allele, d_best_count);
    PGX_HIP(hipGetLastError());
    return PGX_OK;
}

int pgx_runs_load_host(pgx_ctx *ctx, const char *who, const int32_t *a_rows, const int32_t *a_genomes, uint64_t a_records,
                       uint32_t n_alleles, const int32_t *g_rows, const int32_t *g_genomes, uint64_t g_records, uint32_t n_genes,
                       uint32_t n_genomes, const uint32_t *run_start, uint32_t n_runs, const int32_t *gene_of_run,
                       uint64_t *out_duplicates, RunsLoaded *out) {
    // the run arrays are host memory here: refused before anything is uploaded or launched
    const bool records = (a_records == 0 || (a_rows && a_genomes)) && (!gene_of_run || g_records == 0 || (g_rows && g_genomes));
    const char *broken = records ? pgx_runs_host_error(run_start, n_runs, gene_of_run, n_alleles, n_genes) : "NULL record arrays";
    if (broken) {
        pgx_set_error("%s: %s", who, broken);
        return PGX_ERR_INVALID;
    }
    if (out_duplicates) out_duplicates[0] = out_duplicates[1] = 0;
    PGX_HIP(hipSetDevice(ctx->device_id));
    DevBuf d_abits(ctx, RN_SLOT_ABITS), d_acnt(ctx, RN_SLOT_ACNT), d_gbits(ctx, RN_SLOT_GBITS), d_gcnt(ctx, RN_SLOT_GCNT);
    uint64_t dup[2] = {0, 0};
    int rc = pgx_upload_and_build_bitmap(ctx, a_rows, a_genomes, a_records, n_alleles, n_genomes, RN_SLOT_AROWS,
                                         RN_SLOT_AGENOMES, d_abits, d_acnt);
    if (rc == PGX_OK && gene_of_run)
        rc = pgx_upload_and_build_bitmap(ctx, g_rows, g_genomes, g_records, n_genes, n_genomes, RN_SLOT_GROWS, RN_SLOT_GGENOMES,
                                         d_gbits, d_gcnt);
    if (rc == PGX_OK) rc = pgx_read_record_counters(ctx, d_acnt, &dup[0]);
    if (rc == PGX_OK && gene_of_run) rc = pgx_read_record_counters(ctx, d_gcnt, &dup[1]);
    if (rc != PGX_OK) return rc;
    if (out_duplicates) { out_duplicates[0] = dup[0]; out_duplicates[1] = dup[1]; }
    *out = {nullptr, nullptr, nullptr, nullptr, dup[0] || dup[1] || n_runs == 0};   // not 0/1 tables: nothing is computed
    if (out->nothing) return PGX_OK;
    DevPack arrays(ctx, RN_SLOT_IN);
    const PackPart start = arrays.in(run_start, (size_t)n_runs + 1), gene = arrays.in(gene_of_run, n_runs);
    PGX_HIP(arrays.alloc());
    PGX_HIP(arrays.upload(ctx->stream));
    *out = {d_abits.as<uint64_t>(), gene_of_run ? d_gbits.as<uint64_t>() : nullptr, arrays.dev<uint32_t>(start),
            arrays.dev_if(gene_of_run, gene), false};
    return PGX_OK;
}

namespace {

struct RunsOut {
    uint64_t *derived, *diff;
    uint32_t *diff_per_genome, *diff_per_run;
    uint64_t *total;
    int32_t *best_allele;
    uint32_t *best_count;
    bool any() const { return derived || diff || diff_per_genome || diff_per_run || total || best_allele || best_count; }
};

// the checks both entries share, on sizes and pointers only
int runs_args(pgx_ctx *ctx, uint32_t n_alleles, uint32_t n_runs, uint32_t n_genomes, uint32_t n_genes, const void *run_start,
              const RunsOut &out) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(sizes_ok(n_alleles, n_runs, n_genomes, n_genes), "table too large");
    PGX_REQUIRE(n_runs != 0 || !out.any(), "no runs, but outputs requested");
    PGX_REQUIRE(n_runs == 0 || run_start, "NULL run_start");
    return PGX_OK;
}

// Everything on the device; `stream` is synchronised once, at the end (the status word is read back).
int runs_run(pgx_ctx *ctx, const uint64_t *d_abits, uint32_t n_alleles, const uint64_t *d_gbits, uint32_t n_genes,
             uint32_t n_genomes, const uint32_t *d_run_start, uint32_t n_runs, const int32_t *d_gene_of_run, const RunsOut &out,
             void *d_ws, size_t ws_bytes, hipStream_t stream) {
    int rc = runs_args(ctx, n_alleles, n_runs, n_genomes, n_genes, d_run_start, out);
    if (rc != PGX_OK) return rc;
    if (n_runs == 0) return PGX_OK;
    PGX_REQUIRE(d_abits || n_alleles == 0, "NULL allele bitmap");
    const RunsGeom g = make_geom(n_alleles, n_runs, n_genomes);
    PGX_REQUIRE(d_ws && ws_bytes >= g.bytes, "workspace too small (see pgx_allele_runs_workspace_bytes)");
    PGX_REQUIRE(((uintptr_t)d_ws & 15u) == 0, "workspace must be 16-byte aligned");
    HostVec<uint32_t> h_status(ctx, RN_HOST_STATUS, 4);
    if (!h_status.ok()) { pgx_set_error("%s: out of page-locked host memory", __func__); return PGX_ERR_NOMEM; }
    char *p = (char *)d_ws;
    uint32_t *status = (uint32_t *)(p + g.off_status);
    int32_t *counts = (int32_t *)(p + g.off_counts);
    const bool want_diff = out.diff || out.diff_per_genome || out.diff_per_run;
    unsigned long long *diff = want_diff ? (unsigned long long *)(out.diff ? out.diff : (uint64_t *)(p + g.off_diff)) : nullptr;
    const size_t out_bytes = (size_t)n_genomes * g.o_stride * 8;
    const uint32_t run_blocks = ceil_div_u32(n_runs, RN_THREADS);

    PGX_HIP(hipMemsetAsync(status, 0, 16, stream));
    rc = pgx_runs_check_enqueue(ctx, d_run_start, d_gene_of_run, n_runs, n_alleles, n_genes, status, stream);
    if (rc != PGX_OK) return rc;
    if (n_genomes && (out.derived || diff)) {
        if (out.derived) PGX_HIP(hipMemsetAsync(out.derived, 0, out_bytes, stream));
        if (diff) PGX_HIP(hipMemsetAsync(diff, 0, out_bytes, stream));
        const uint32_t slabs = std::min(ceil_div_u32(n_genomes, RN_SLAB), 65535u);
        ProfScope prof(ctx, "runs_or_kernel", stream);
        runs_or_kernel<<<dim3(run_blocks, slabs), RN_THREADS, 0, stream>>>(
            (const unsigned long long *)d_abits, g.a_stride, n_alleles, d_run_start, n_runs, (const unsigned long long *)d_gbits,
            pgx_bitmap_stride_words(n_genes), n_genes, d_gene_of_run, n_genomes, g.o_stride, (unsigned long long *)out.derived, diff);
    }
    PGX_HIP(hipGetLastError());
    if (out.diff_per_run) {
        rc = pgx_row_counts_dev(ctx, (const uint64_t *)diff, n_runs, n_genomes, (int32_t *)out.diff_per_run, stream);
        if (rc != PGX_OK) return rc;
    }
    if (out.diff_per_genome && n_genomes) {
        ProfScope prof(ctx, "runs_genome_kernel", stream);
        runs_genome_kernel<<<n_genomes, RN_THREADS, 0, stream>>>(diff, g.o_stride, out.diff_per_genome);
        PGX_HIP(hipGetLastError());
    }
    if (out.total || out.best_allele || out.best_count) {
        rc = pgx_runs_stats_enqueue(ctx, d_abits, n_alleles, n_genomes, d_run_start, n_runs, counts, out.total, out.best_allele,
                                    out.best_count, stream);
        if (rc != PGX_OK) return rc;
    }
    PGX_HIP(hipMemcpyAsync(h_status.data(), status, 4, hipMemcpyDeviceToHost, stream));
    PGX_HIP(hipStreamSynchronize(stream));
    const char *broken = pgx_runs_status_error(h_status[0]);
    PGX_REQUIRE(!broken, broken);
    return PGX_OK;
}

int runs_host(pgx_ctx *ctx, const int32_t *a_rows, const int32_t *a_genomes, uint64_t a_records, uint32_t n_alleles,
              const int32_t *g_rows, const int32_t *g_genomes, uint64_t g_records, uint32_t n_genes, uint32_t n_genomes,
              const uint32_t *run_start, uint32_t n_runs, const int32_t *gene_of_run, const RunsOut &out,
              uint64_t *out_duplicates) {
    int rc = runs_args(ctx, n_alleles, n_runs, n_genomes, n_genes, run_start, out);
    if (rc != PGX_OK) return rc;
    RunsLoaded in;
    rc = pgx_runs_load_host(ctx, __func__, a_rows, a_genomes, a_records, n_alleles, g_rows, g_genomes, g_records, n_genes,
                            n_genomes, run_start, n_runs, gene_of_run, out_duplicates, &in);
    if (rc != PGX_OK || in.nothing) return rc;
    const RunsGeom g = make_geom(n_alleles, n_runs, n_genomes);
    const size_t bitmap_words = (size_t)n_genomes * g.o_stride;
    DevBuf d_ws(ctx, RN_SLOT_WS);
    DevPack res(ctx, RN_SLOT_OUT);                            // a bitmap that was not asked for takes no room
    const PackPart derived = res.out(out.derived, out.derived ? bitmap_words : 0),
                   diff = res.out(out.diff, out.diff ? bitmap_words : 0),
                   per_genome = res.out(out.diff_per_genome, n_genomes), per_run = res.out(out.diff_per_run, n_runs),
                   total = res.out(out.total, n_runs), best = res.out(out.best_allele, n_runs),
                   best_count = res.out(out.best_count, n_runs);
    PGX_HIP(d_ws.alloc(g.bytes));
    PGX_HIP(res.alloc());
    const RunsOut dev = {res.dev_if(out.derived, derived), res.dev_if(out.diff, diff), res.dev_if(out.diff_per_genome, per_genome),
                         res.dev_if(out.diff_per_run, per_run), res.dev_if(out.total, total), res.dev_if(out.best_allele, best),
                         res.dev_if(out.best_count, best_count)};
    rc = runs_run(ctx, in.d_abits, n_alleles, in.d_gbits, n_genes, n_genomes, in.d_run_start, n_runs, in.d_gene_of_run, dev,
                  d_ws.p, g.bytes, ctx->stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(res.download(ctx->stream));
    PGX_HIP(hipStreamSynchronize(ctx->stream));
    return PGX_OK;
}

}  // namespace

extern "C" {

size_t pgx_allele_runs_workspace_bytes(uint32_t n_alleles, uint32_t n_runs, uint32_t n_genomes) {
    if (!sizes_ok(n_alleles, n_runs, n_genomes, 0)) return 0;
    return make_geom(n_alleles, n_runs, n_genomes).bytes;
}

int pgx_allele_runs(pgx_ctx *ctx, const int32_t *allele_rows, const int32_t *allele_genomes, uint64_t n_allele_records,
                    uint32_t n_alleles, const int32_t *gene_rows, const int32_t *gene_genomes, uint64_t n_gene_records,
                    uint32_t n_genes, uint32_t n_genomes, const uint32_t *run_start, uint32_t n_runs, const int32_t *gene_of_run,
                    uint64_t *out_derived, uint64_t *out_diff, uint32_t *out_diff_per_genome, uint32_t *out_diff_per_run,
                    uint64_t *out_total, int32_t *out_best_allele, uint32_t *out_best_count, uint64_t *out_duplicates) {
    return guarded(__func__, [&] {
        const RunsOut out = {out_derived, out_diff, out_diff_per_genome, out_diff_per_run, out_total, out_best_allele,
                             out_best_count};
        return runs_host(ctx, allele_rows, allele_genomes, n_allele_records, n_alleles, gene_rows, gene_genomes, n_gene_records,
                         n_genes, n_genomes, run_start, n_runs, gene_of_run, out, out_duplicates);
    });
}

int pgx_allele_runs_dev(pgx_ctx *ctx, const uint64_t *d_allele_bits, uint32_t n_alleles, const uint64_t *d_gene_bits,
                        uint32_t n_genes, uint32_t n_genomes, const uint32_t *d_run_start, uint32_t n_runs,
                        const int32_t *d_gene_of_run, uint64_t *d_derived, uint64_t *d_diff, uint32_t *d_diff_per_genome,
                        uint32_t *d_diff_per_run, uint64_t *d_total, int32_t *d_best_allele, uint32_t *d_best_count,
                        void *d_workspace, size_t workspace_bytes, void *stream) {
    return guarded(__func__, [&] {
        const RunsOut out = {d_derived, d_diff, d_diff_per_genome, d_diff_per_run, d_total, d_best_allele, d_best_count};
        return runs_run(ctx, d_allele_bits, n_alleles, d_gene_bits, n_genes, n_genomes, d_run_start, n_runs, d_gene_of_run, out,
                        d_workspace, workspace_bytes, (hipStream_t)stream);
    });
}

}  // extern "C"
