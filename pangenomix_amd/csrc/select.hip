// Core / dominant allele selection on the genome-major bitmaps (reference core_genome.py:7-26 create_core_genes_fasta and
// allele_identification.py:7-20 create_alleles_fasta, whose chains are iterrows() loops over two pandas frames): for the runs
// of allele rows that runs.hip defines,
//   gene_count[r]  = set bits of row gene_of_run[r] of the gene table (0 without one)
//   best_allele[r] = the first row of the run with the largest occupancy count (runs.hip computes it, called from here)
//   mask[r]        bit t: the run is eligible (it has a best allele and, when gene_of_run is given, a gene row) and
//                  gene_count[r] >= thresholds[t]
//   selected[t][]  = best_allele[r] of the runs with bit t, in ascending r; n_selected[t] how many
// for up to 32 thresholds in one pass.
//
// Kernels (plain launches on one stream; no atomics on a result and no workgroup waits for another, so the same inputs
// give the same bytes whatever order the waves run in):
//   row_counts_kernel     (pancore.hip) the gene rows' counts;   runs_stats_kernel (runs.hip) best_allele / best_count
//   select_mask_kernel    one lane per run, CS_BLOCK runs per workgroup: gene_count and mask; per threshold ONE 64-bit
//                         __ballot of the wave's bit t, whose popcount lane 0 leaves in LDS; lanes t < n_thresholds add the
//                         waves' counts and store the workgroup's total [block][t]
//   select_scan_kernel    workgroup t makes the exclusive scan over the workgroups' totals of threshold t in place, CS_BLOCK
//                         at a time with a carry (__shfl_up inside a wave, the waves' sums through LDS), and n_selected[t]
//   select_scatter_kernel the same ballots from the stored masks; the waves' counts are scanned (exclusive) in LDS; a lane
//                         with bit t writes best_allele[r] at  block offset + wave offset + set bits below its lane
//   runs_check_kernel     (runs.hip) the device entry's check of the caller's run arrays; everything above clamps what it
//                         reads (a gene row out of range counts as none), so that bad arrays never become a bad address
#include "pgx_internal.h"

namespace {

constexpr int CS_BLOCK = 256;                       // runs per workgroup (pgx_core_select_block)
constexpr int CS_WAVES = CS_BLOCK / 64;
constexpr uint32_t CS_MAX_THRESHOLDS = 32;

struct SelectGeom {
    uint32_t n_blocks;
    size_t off_acounts, off_gcounts, off_best, off_mask, off_totals, off_nsel, off_status, bytes;
};

SelectGeom make_geom(uint32_t n_alleles, uint32_t n_genes, uint32_t n_runs) {
    SelectGeom g;
    g.n_blocks = ceil_div_u32(n_runs, CS_BLOCK);
    WsLayout ws;
    g.off_acounts = ws.take((size_t)n_alleles * 4);
    g.off_gcounts = ws.take((size_t)n_genes * 4);
    g.off_best = ws.take((size_t)n_runs * 4);
    g.off_mask = ws.take((size_t)n_runs * 4);
    g.off_totals = ws.take((size_t)g.n_blocks * CS_MAX_THRESHOLDS * 4);
    g.off_nsel = ws.take(CS_MAX_THRESHOLDS * 4);
    g.off_status = ws.take(16);
    g.bytes = ws.off;
    return g;
}

bool sizes_ok(uint32_t n_alleles, uint32_t n_runs, uint32_t n_genomes, uint32_t n_genes) {
    return n_alleles < (1u << 31) && n_runs < (1u << 31) && n_genomes < (1u << 31) && n_genes < (1u << 31);
}

// gene_count / mask of the workgroup's runs; totals[block][t] = its runs with bit t (totals may be NULL). Whole waves ballot:
// lanes beyond n_runs carry mask 0.
__global__ __launch_bounds__(CS_BLOCK) void select_mask_kernel(const int32_t *__restrict__ best_allele,
                                                               const int32_t *__restrict__ gene_of_run,
                                                               const int32_t *__restrict__ gene_counts, uint32_t n_genes,
                                                               uint32_t n_runs, const uint32_t *__restrict__ thresholds,
                                                               uint32_t n_thresholds, uint32_t *__restrict__ gene_count,
                                                               uint32_t *__restrict__ mask, uint32_t *__restrict__ totals) {
    __shared__ uint32_t thr[CS_MAX_THRESHOLDS];
    __shared__ uint32_t wave_count[CS_MAX_THRESHOLDS][CS_WAVES];
    const uint32_t r = blockIdx.x * CS_BLOCK + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x < n_thresholds) thr[threadIdx.x] = thresholds[threadIdx.x];
    __syncthreads();
    uint32_t m = 0;
    if (r < n_runs) {
        const bool some = best_allele && best_allele[r] >= 0;
        bool has_gene = true;
        uint32_t count = 0;
        if (gene_of_run) {
            const uint32_t gene = (uint32_t)gene_of_run[r];               // (-1 and anything out of range: no gene row)
            has_gene = gene < n_genes;
            if (has_gene && gene_counts) count = (uint32_t)gene_counts[gene];
        }
        if (some && has_gene)
            for (uint32_t t = 0; t < n_thresholds; ++t) m |= (count >= thr[t] ? 1u : 0u) << t;
        if (gene_count) gene_count[r] = count;
        if (mask) mask[r] = m;
    }
    if (!totals) return;
    for (uint32_t t = 0; t < n_thresholds; ++t) {
        const unsigned long long hit = __ballot((m >> t) & 1u);
        if (lane == 0) wave_count[t][wave] = (uint32_t)__popcll(hit);
    }
    __syncthreads();
    if (threadIdx.x < n_thresholds) {
        uint32_t sum = 0;
        for (int w = 0; w < CS_WAVES; ++w) sum += wave_count[threadIdx.x][w];
        totals[(size_t)blockIdx.x * CS_MAX_THRESHOLDS + threadIdx.x] = sum;
    }
}

// totals[b][t] -> the runs with bit t in the workgroups before b, for t = blockIdx.x; n_selected[t] = all of them
__global__ __launch_bounds__(CS_BLOCK) void select_scan_kernel(uint32_t *__restrict__ totals, uint32_t n_blocks,
                                                               uint32_t *__restrict__ n_selected) {
    __shared__ uint32_t wave_sum[CS_WAVES];
    const uint32_t t = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_blocks; base += CS_BLOCK) {          // (uniform: every lane takes every round)
        const uint32_t b = base + threadIdx.x;
        const uint32_t v = b < n_blocks ? totals[(size_t)b * CS_MAX_THRESHOLDS + t] : 0u;
        uint32_t incl = v;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= (uint32_t)d) incl += up;
        }
        if (lane == 63u) wave_sum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t w = 0; w < (uint32_t)CS_WAVES; ++w) {
            if (w < wave) before += wave_sum[w];
            all += wave_sum[w];
        }
        if (b < n_blocks) totals[(size_t)b * CS_MAX_THRESHOLDS + t] = carry + before + incl - v;
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) n_selected[t] = carry;
}

// selected[t][offsets[block][t] + rank of the run among the workgroup's runs with bit t] = best_allele[r]
__global__ __launch_bounds__(CS_BLOCK) void select_scatter_kernel(const uint32_t *__restrict__ mask,
                                                                  const int32_t *__restrict__ best_allele, uint32_t n_runs,
                                                                  uint32_t n_thresholds, const uint32_t *__restrict__ offsets,
                                                                  int32_t *__restrict__ selected) {
    __shared__ uint32_t wave_off[CS_MAX_THRESHOLDS][CS_WAVES];
    const uint32_t r = blockIdx.x * CS_BLOCK + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t m = r < n_runs ? mask[r] : 0u;
    for (uint32_t t = 0; t < n_thresholds; ++t) {
        const unsigned long long hit = __ballot((m >> t) & 1u);
        if (lane == 0) wave_off[t][wave] = (uint32_t)__popcll(hit);
    }
    __syncthreads();
    if (threadIdx.x < n_thresholds) {                                     // exclusive scan of the waves' counts, in LDS
        uint32_t run = 0;
        for (int w = 0; w < CS_WAVES; ++w) {
            const uint32_t c = wave_off[threadIdx.x][w];
            wave_off[threadIdx.x][w] = run;
            run += c;
        }
    }
    __syncthreads();
    const int32_t best = m ? best_allele[r] : -1;                         // (m != 0 only for r < n_runs)
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint32_t t = 0; t < n_thresholds; ++t) {
        const unsigned long long hit = __ballot((m >> t) & 1u);
        if ((m >> t) & 1u) {
            const uint32_t pos = offsets[(size_t)blockIdx.x * CS_MAX_THRESHOLDS + t] + wave_off[t][wave] +
                                 (uint32_t)__popcll(hit & below);
            selected[(size_t)t * n_runs + pos] = best;
        }
    }
}

struct SelectOut {
    uint32_t *gene_count;
    int32_t *best_allele;
    uint32_t *best_count, *mask;
    int32_t *selected;
    uint32_t *n_selected;
    bool any() const { return gene_count || best_allele || best_count || mask || selected || n_selected; }
};

// the checks both entries share, on sizes and pointers only
int select_args(pgx_ctx *ctx, uint32_t n_alleles, uint32_t n_runs, uint32_t n_genomes, uint32_t n_genes, const void *run_start,
                const void *thresholds, uint32_t n_thresholds, const SelectOut &out) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(sizes_ok(n_alleles, n_runs, n_genomes, n_genes), "table too large");
    PGX_REQUIRE(n_thresholds >= 1 && n_thresholds <= CS_MAX_THRESHOLDS, "n_thresholds must be 1..32");
    PGX_REQUIRE(thresholds, "NULL thresholds");
    PGX_REQUIRE(n_runs != 0 || !out.any(), "no runs, but outputs requested");
    PGX_REQUIRE(n_runs == 0 || run_start, "NULL run_start");
    return PGX_OK;
}

// Everything on the device; `stream` is synchronised once, at the end (the status word is read back).
int select_run(pgx_ctx *ctx, const uint64_t *d_abits, uint32_t n_alleles, const uint64_t *d_gbits, uint32_t n_genes,
               uint32_t n_genomes, const uint32_t *d_run_start, uint32_t n_runs, const int32_t *d_gene_of_run,
               const uint32_t *d_thresholds, uint32_t n_thresholds, const SelectOut &out, void *d_ws, size_t ws_bytes,
               hipStream_t stream) {
    int rc = select_args(ctx, n_alleles, n_runs, n_genomes, n_genes, d_run_start, d_thresholds, n_thresholds, out);
    if (rc != PGX_OK) return rc;
    if (n_runs == 0) return PGX_OK;
    PGX_REQUIRE(d_abits || n_alleles == 0, "NULL allele bitmap");
    const SelectGeom g = make_geom(n_alleles, n_genes, n_runs);
    PGX_REQUIRE(d_ws && ws_bytes >= g.bytes, "workspace too small (see pgx_core_select_workspace_bytes)");
    PGX_REQUIRE(((uintptr_t)d_ws & 15u) == 0, "workspace must be 16-byte aligned");
    HostVec<uint32_t> h_status(ctx, CS_HOST_STATUS, 4);
    if (!h_status.ok()) { pgx_set_error("%s: out of page-locked host memory", __func__); return PGX_ERR_NOMEM; }
    char *p = (char *)d_ws;
    uint32_t *status = (uint32_t *)(p + g.off_status);
    const bool want_scan = out.selected || out.n_selected;
    const bool want_mask = out.mask || want_scan;
    const bool want_best = out.best_allele || out.best_count || want_mask;
    const bool want_gene = (out.gene_count || want_mask) && d_gbits && d_gene_of_run && n_genes;
    int32_t *best = out.best_allele ? out.best_allele : (int32_t *)(p + g.off_best);
    uint32_t *mask = out.mask ? out.mask : (uint32_t *)(p + g.off_mask);
    uint32_t *totals = (uint32_t *)(p + g.off_totals);
    uint32_t *n_selected = out.n_selected ? out.n_selected : (uint32_t *)(p + g.off_nsel);
    int32_t *gene_counts = (int32_t *)(p + g.off_gcounts);

    PGX_HIP(hipMemsetAsync(status, 0, 16, stream));
    rc = pgx_runs_check_enqueue(ctx, d_run_start, d_gene_of_run, n_runs, n_alleles, n_genes, status, stream);
    if (rc != PGX_OK) return rc;
    if (want_best) {
        rc = pgx_runs_stats_enqueue(ctx, d_abits, n_alleles, n_genomes, d_run_start, n_runs, (int32_t *)(p + g.off_acounts),
                                    nullptr, best, out.best_count, stream);
        if (rc != PGX_OK) return rc;
    }
    if (want_gene) {
        rc = pgx_row_counts_dev(ctx, d_gbits, n_genes, n_genomes, gene_counts, stream);
        if (rc != PGX_OK) return rc;
    }
    if (out.gene_count || want_mask) {
        ProfScope prof(ctx, "select_mask_kernel", stream);
        select_mask_kernel<<<g.n_blocks, CS_BLOCK, 0, stream>>>(want_mask ? best : nullptr, d_gene_of_run,
                                                                want_gene ? gene_counts : nullptr, n_genes, n_runs,
                                                                d_thresholds, n_thresholds, out.gene_count,
                                                                want_mask ? mask : nullptr, want_scan ? totals : nullptr);
        PGX_HIP(hipGetLastError());
    }
    if (want_scan) {
        ProfScope prof(ctx, "select_scan_kernel", stream);
        select_scan_kernel<<<n_thresholds, CS_BLOCK, 0, stream>>>(totals, g.n_blocks, n_selected);
        PGX_HIP(hipGetLastError());
    }
    if (out.selected) {
        ProfScope prof(ctx, "select_scatter_kernel", stream);
        select_scatter_kernel<<<g.n_blocks, CS_BLOCK, 0, stream>>>(mask, best, n_runs, n_thresholds, totals, out.selected);
        PGX_HIP(hipGetLastError());
    }
    PGX_HIP(hipMemcpyAsync(h_status.data(), status, 4, hipMemcpyDeviceToHost, stream));
    PGX_HIP(hipStreamSynchronize(stream));
    const char *broken = pgx_runs_status_error(h_status[0]);
    PGX_REQUIRE(!broken, broken);
    return PGX_OK;
}

int select_host(pgx_ctx *ctx, const int32_t *a_rows, const int32_t *a_genomes, uint64_t a_records, uint32_t n_alleles,
                const int32_t *g_rows, const int32_t *g_genomes, uint64_t g_records, uint32_t n_genes, uint32_t n_genomes,
                const uint32_t *run_start, uint32_t n_runs, const int32_t *gene_of_run, const uint32_t *thresholds,
                uint32_t n_thresholds, const SelectOut &out, uint64_t *out_duplicates) {
    int rc = select_args(ctx, n_alleles, n_runs, n_genomes, n_genes, run_start, thresholds, n_thresholds, out);
    if (rc != PGX_OK) return rc;
    RunsLoaded in;
    rc = pgx_runs_load_host(ctx, __func__, a_rows, a_genomes, a_records, n_alleles, g_rows, g_genomes, g_records, n_genes,
                            n_genomes, run_start, n_runs, gene_of_run, out_duplicates, &in);
    if (rc != PGX_OK || in.nothing) return rc;
    const SelectGeom g = make_geom(n_alleles, n_genes, n_runs);
    DevBuf d_ws(ctx, CS_SLOT_WS);
    DevPack thr(ctx, CS_SLOT_THR), res(ctx, CS_SLOT_OUT);
    // n_selected and the rows of `selected` are fetched below, as far as they were written
    const PackPart thr_part = thr.in(thresholds, n_thresholds), gene_count = res.out(out.gene_count, n_runs),
                   best = res.out(out.best_allele, n_runs), best_count = res.out(out.best_count, n_runs),
                   mask = res.out(out.mask, n_runs), nsel = res.out<uint32_t>(nullptr, CS_MAX_THRESHOLDS),
                   sel = res.out<int32_t>(nullptr, out.selected ? (size_t)n_runs * n_thresholds : 0);
    PGX_HIP(d_ws.alloc(g.bytes));
    PGX_HIP(thr.alloc());
    PGX_HIP(res.alloc());
    PGX_HIP(thr.upload(ctx->stream));
    const SelectOut dev = {res.dev_if(out.gene_count, gene_count), res.dev_if(out.best_allele, best),
                           res.dev_if(out.best_count, best_count), res.dev_if(out.mask, mask), res.dev_if(out.selected, sel),
                           (out.selected || out.n_selected) ? res.dev<uint32_t>(nsel) : nullptr};
    rc = select_run(ctx, in.d_abits, n_alleles, in.d_gbits, n_genes, n_genomes, in.d_run_start, n_runs, in.d_gene_of_run,
                    thr.dev<uint32_t>(thr_part), n_thresholds, dev, d_ws.p, g.bytes, ctx->stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(res.download(ctx->stream));
    uint32_t n_sel[CS_MAX_THRESHOLDS] = {0};
    if (dev.n_selected) {
        PGX_HIP(res.download(nsel, 0, n_thresholds, n_sel, ctx->stream));
        PGX_HIP(hipStreamSynchronize(ctx->stream));
        if (out.n_selected) memcpy(out.n_selected, n_sel, (size_t)n_thresholds * 4);
    }
    for (uint32_t t = 0; out.selected && t < n_thresholds; ++t)
        PGX_HIP(res.download(sel, (size_t)t * n_runs, std::min(n_sel[t], n_runs), out.selected + (size_t)t * n_runs, ctx->stream));
    PGX_HIP(hipStreamSynchronize(ctx->stream));
    return PGX_OK;
}

}  // namespace

extern "C" {

uint32_t pgx_core_select_block(void) { return CS_BLOCK; }

size_t pgx_core_select_workspace_bytes(uint32_t n_alleles, uint32_t n_genes, uint32_t n_runs) {
    if (!sizes_ok(n_alleles, n_runs, 0, n_genes)) return 0;
    return make_geom(n_alleles, n_genes, n_runs).bytes;
}

int pgx_core_select(pgx_ctx *ctx, const int32_t *allele_rows, const int32_t *allele_genomes, uint64_t n_allele_records,
                    uint32_t n_alleles, const int32_t *gene_rows, const int32_t *gene_genomes, uint64_t n_gene_records,
                    uint32_t n_genes, uint32_t n_genomes, const uint32_t *run_start, uint32_t n_runs, const int32_t *gene_of_run,
                    const uint32_t *thresholds, uint32_t n_thresholds, uint32_t *out_gene_count, int32_t *out_best_allele,
                    uint32_t *out_best_count, uint32_t *out_mask, int32_t *out_selected, uint32_t *out_n_selected,
                    uint64_t *out_duplicates) {
    return guarded(__func__, [&] {
        const SelectOut out = {out_gene_count, out_best_allele, out_best_count, out_mask, out_selected, out_n_selected};
        return select_host(ctx, allele_rows, allele_genomes, n_allele_records, n_alleles, gene_rows, gene_genomes, n_gene_records,
                           n_genes, n_genomes, run_start, n_runs, gene_of_run, thresholds, n_thresholds, out, out_duplicates);
    });
}

int pgx_core_select_dev(pgx_ctx *ctx, const uint64_t *d_allele_bits, uint32_t n_alleles, const uint64_t *d_gene_bits,
                        uint32_t n_genes, uint32_t n_genomes, const uint32_t *d_run_start, uint32_t n_runs,
                        const int32_t *d_gene_of_run, const uint32_t *d_thresholds, uint32_t n_thresholds,
                        uint32_t *d_gene_count, int32_t *d_best_allele, uint32_t *d_best_count, uint32_t *d_mask,
                        int32_t *d_selected, uint32_t *d_n_selected, void *d_workspace, size_t workspace_bytes, void *stream) {
    return guarded(__func__, [&] {
        const SelectOut out = {d_gene_count, d_best_allele, d_best_count, d_mask, d_selected, d_n_selected};
        return select_run(ctx, d_allele_bits, n_alleles, d_gene_bits, n_genes, n_genomes, d_run_start, n_runs, d_gene_of_run,
                          d_thresholds, n_thresholds, out, d_workspace, workspace_bytes, (hipStream_t)stream);
    });
}

}  // extern "C"
