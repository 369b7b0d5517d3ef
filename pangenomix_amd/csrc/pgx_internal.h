// Internal helpers shared by the libpgx translation units (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "../../include/pgx.h"
#include "pgx_guard.h"
#include "pgx_pack.h"

#include <string>
#include <utility>
#include <algorithm>
#include <cstdlib>
#include <vector>

// Optional per-kernel timing (pgx_profile_*): HIP events recorded on the launch stream
// around each kernel, resolved when the caller reads the slots.
struct ProfSlot {
    std::string name;
    double total_ms = 0.0;
    uint64_t launches = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

// Every buffer a context keeps between calls lives in one of three grow-only tables, and every slot of a table has ONE
// name, here: two users of one slot silently overwrite (or reallocate) each other's data. To add a buffer, add an
// enumerator to its module's group; DevBuf, HostVec and Pinned take nothing but these types.
enum DevSlot : int {        // pgx_ctx::arena, through DevBuf
    // cluster.hip: pgx_cluster_greedy_dev, then the two upload buffers of pgx_cluster_greedy
    CL_SLOT_IN_LEN = 0, CL_SLOT_RES, CL_SLOT_OFF, CL_SLOT_LEN, CL_SLOT_WCODE, CL_SLOT_WMULT, CL_SLOT_WCNT, CL_SLOT_AA1,
    CL_SLOT_AAS, CL_SLOT_AAN, CL_SLOT_LINES, CL_SLOT_POOL0, CL_SLOT_POOL1, CL_SLOT_IDX, CL_SLOT_NEWBITS, CL_SLOT_TOUCHED,
    CL_SLOT_FIRST, CL_SLOT_BEST_OWN, CL_SLOT_RCVIS, CL_SLOT_COUNTERS, CL_SLOT_VISITS, CL_SLOT_PAIRS_W, CL_SLOT_PAIRS_K,
    CL_SLOT_BLK_LIST, CL_SLOT_ULIST, CL_SLOT_NEW_LIST, CL_SLOT_FLAGS, CL_SLOT_GSCRATCH, CL_SLOT_ORDER, CL_SLOT_LIST,
    CL_SLOT_GATHER, CL_SLOT_PK, CL_SLOT_PKOFF, CL_SLOT_COUNTERS2, CL_SLOT_BEST2, CL_SLOT_FLAGS2, CL_SLOT_PAIRS_W2,
    CL_SLOT_GSCRATCH2, CL_SLOT_THR, CL_SLOT_HUGEWORDS, CL_SLOT_XSEND, CL_SLOT_XRECV, CL_SLOT_HIST, CL_SLOT_SORTCNT,
    CL_SLOT_TILESUM, CL_SLOT_RUNS, CL_SLOT_UP_RES, CL_SLOT_UP_OFF,
    // pancore.hip; PGX_SLOT_RESIDENT is the pipeline's resident bitmap (pgx_resident_bitmap)
    PC_SLOT_ROWS, PC_SLOT_GENOMES, PC_SLOT_BITS, PC_SLOT_PERMS, PC_SLOT_PAN, PC_SLOT_CORE, PC_SLOT_WS, PC_SLOT_CNT,
    PC_SLOT_COUNTS, PC_SLOT_TABLE, PGX_SLOT_RESIDENT, PC_SLOT_RES_A, PC_SLOT_RES_B, PC_SLOT_RES_C, PC_SLOT_RES_D,
    // heaps.hip
    HP_SLOT_TAB, HP_SLOT_A, HP_SLOT_K,
    // bernoulli.hip; PGX_SLOT_BERN_BITS is the table pgx_bernoulli_load* left, read in place by bernoulli_cd.hip
    PGX_SLOT_BERN_BITS, BN_SLOT_ROWS, BN_SLOT_GENOMES, BN_SLOT_CNT, BN_SLOT_MAP, BN_SLOT_PQ, BN_SLOT_OUT, BN_SLOT_WS,
    // betabinom.hip
    BB_SLOT_WORDS0, BB_SLOT_WORDS1, BB_SLOT_CDF, BB_SLOT_MODEL, BB_SLOT_KS, BB_SLOT_HIST, BB_SLOT_IDX,
    // fcd.hip
    FC_SLOT_BITS, FC_SLOT_ROWS, FC_SLOT_GENOMES, FC_SLOT_CNT, FC_SLOT_WS, FC_SLOT_MAP, FC_SLOT_CMAP, FC_SLOT_CROWS,
    FC_SLOT_CCOLS, FC_SLOT_CLEARED,
    // fcd_match.hip: the uploaded lists, the workspace, the results, the whole overlap matrix when it is asked for
    FC_SLOT_M_LISTS, FC_SLOT_M_WS, FC_SLOT_M_OUT, FC_SLOT_M_MATRIX,
    // assoc.hip: the table, the workspace, the maps and masks in one, every result in one
    AS_SLOT_BITS, AS_SLOT_ROWS, AS_SLOT_GENOMES, AS_SLOT_CNT, AS_SLOT_WS, AS_SLOT_IN, AS_SLOT_OUT,
    // runs.hip: the allele table and the gene table, run_start and gene_of_run in one (pgx_runs_load_host fills these for
    // select.hip too), then its own workspace and every result in one
    RN_SLOT_ABITS, RN_SLOT_AROWS, RN_SLOT_AGENOMES, RN_SLOT_ACNT, RN_SLOT_GBITS, RN_SLOT_GROWS, RN_SLOT_GGENOMES,
    RN_SLOT_GCNT, RN_SLOT_IN, RN_SLOT_WS, RN_SLOT_OUT,
    // select.hip: the workspace, the thresholds, every result in one
    CS_SLOT_WS, CS_SLOT_THR, CS_SLOT_OUT,
    // scan.hip
    SC_SLOT_TEXT, SC_SLOT_KEYS, SC_SLOT_FOUND, SC_SLOT_WS,
    // bernoulli_cd.hip
    CD_SLOT_INIT, CD_SLOT_TABLE, CD_SLOT_SOLVER, CD_SLOT_WS,
    // dict.hip: the loaded set stays in the first three; then pgx_genome_sets_diff
    DM_SLOT_KEYS, DM_SLOT_KEY_OFF, DM_SLOT_TABLE, DM_SLOT_QUERIES, DM_SLOT_QUERY_OFF, DM_SLOT_OUT,
    SD_SLOT_ROWS, SD_SLOT_GENOMES, SD_SLOT_A_BITS, SD_SLOT_A_CNT, SD_SLOT_B_BITS, SD_SLOT_B_CNT, SD_SLOT_OUT,
    // svm.hip: the table, the workspace (Gram matrices, status), every uploaded input in one, every result in one
    SV_SLOT_BITS, SV_SLOT_ROWS, SV_SLOT_GENOMES, SV_SLOT_CNT, SV_SLOT_WS, SV_SLOT_IN, SV_SLOT_OUT,
    // prox.hip: pgx_prox_cut (the text, the window arrays in one, output and bad flags in one), then pgx_prox_group (the
    // blob, offsets and genes in one, the workspace, every result in one)
    PX_SLOT_TEXT, PX_SLOT_WINDOWS, PX_SLOT_OUT, PX_SLOT_BLOB, PX_SLOT_RECORDS, PX_SLOT_WS, PX_SLOT_RESULT,
    // annot.hip: the ids, row and run offsets in one, the workspace, every result in one
    AN_SLOT_TOK, AN_SLOT_OFFSETS, AN_SLOT_WS, AN_SLOT_RESULT,
    // reach.hip: the graph, targets and sources in one, the two mask buffers and the flag, the lengths
    GR_SLOT_IN, GR_SLOT_WS, GR_SLOT_OUT,
    // terms.hip: the text, the windows and the terms in one, the masks
    TS_SLOT_TEXT, TS_SLOT_IN, TS_SLOT_OUT,
    // mic.hip: pgx_tuple_group (the columns, the workspace, every result in one), then pgx_mic_infer (the case tables in
    // one, the row arrays in one, the codes)
    TG_SLOT_IN, TG_SLOT_WS, TG_SLOT_OUT, MI_SLOT_TABLES, MI_SLOT_ROWS, MI_SLOT_OUT,
    // tree.hip: the species' table, the tree arrays in one, counts and totals in one
    TR_SLOT_BITS, TR_SLOT_ROWS, TR_SLOT_SPECIES, TR_SLOT_CNT, TR_SLOT_IN, TR_SLOT_OUT,
    // pattern.hip: the loaded set stays in the first three (blob, offsets, table and filter); then a query's text and its
    // first and count in one
    PT_SLOT_PATTERNS, PT_SLOT_OFFSETS, PT_SLOT_WS, PT_SLOT_TEXT, PT_SLOT_OUT,
    // near.hip: the loaded set stays in the first four (blob, offsets, max_mismatch, table and filter); then a query's text,
    // its active flags and its best
    NR_SLOT_PATTERNS, NR_SLOT_OFFSETS, NR_SLOT_MISMATCH, NR_SLOT_WS, NR_SLOT_TEXT, NR_SLOT_ACTIVE, NR_SLOT_OUT,
    // sw.hip: the two sets' residues, offsets, pairs, thresholds and order in one, the workspace, the results
    SW_SLOT_RES1, SW_SLOT_RES2, SW_SLOT_IN, SW_SLOT_WS, SW_SLOT_OUT,
    DEV_SLOT_COUNT
};
enum HostSlot : int {       // pgx_ctx::host_scratch, through HostVec
    // cluster.hip
    CL_HOST_IN_LEN = 0, CL_HOST_ORDER, CL_HOST_OFF, CL_HOST_LEN, CL_HOST_THR, CL_HOST_HIST, CL_HOST_RUNS, CL_HOST_WCNT,
    CL_HOST_CLUSTER_OF, CL_HOST_IDEN_OF, CL_HOST_STRAND_OF,
    PGX_HOST_STAGE,         // pgx_core.hip: the staging buffers of pgx_staged_h2d
    BB_HOST_WORDS0, BB_HOST_WORDS1, BB_HOST_IDX,
    FC_HOST_RES,
    AS_HOST_STATUS,
    RN_HOST_STATUS,
    CS_HOST_STATUS,
    SV_HOST_STATUS,
    PX_HOST_OFFSETS,
    HOST_SLOT_COUNT
};
enum PinSlot : int {        // pgx_ctx::host_arena, through Pinned (cluster.hip)
    CL_PIN_W = 0, CL_PIN_K, CL_PIN_BEST, CL_PIN_CNT, CL_PIN_BLK, CL_PIN_NEW, CL_PIN_RCVIS, CL_PIN_LIST, CL_PIN_GATHER,
    CL_PIN_PUSH, CL_PIN_W2, CL_PIN_BEST2, CL_PIN_CCNT, CL_PIN_CCNT2, CL_PIN_TAKEN,
    PIN_SLOT_COUNT
};

struct pgx_ctx {
    int device_id;
    hipStream_t stream;  // used by the host-pointer entry points
    hipStream_t stream2; // side stream: next sweep's index + table pass overlap the current sweep
    hipEvent_t ev_main = nullptr, ev_side[2] = {nullptr, nullptr};
    hipDeviceProp_t prop;
    bool profiling = false;
    std::vector<ProfSlot> prof;
    std::vector<hipEvent_t> event_pool;
    // grow-only device workspace, reused by successive calls on this context (slot -> buffer)
    std::pair<void *, size_t> arena[DEV_SLOT_COUNT] = {};
    // grow-only coherent page-locked host buffers (slot -> buffer), same idea
    std::pair<void *, size_t> host_arena[PIN_SLOT_COUNT] = {};
    // grow-only page-locked host scratch (slot -> buffer): the per-sequence arrays of a clustering call
    // (tens of MB) are neither allocated, faulted in nor freed again by every call, and their copies to
    // and from the device are asynchronous (from pageable memory every hipMemcpyAsync blocked the host)
    std::pair<void *, size_t> host_scratch[HOST_SLOT_COUNT] = {};
    std::vector<hipEvent_t> stage_events;   // pgx_staged_h2d: one per staging buffer (its last DMA)
    // the gene x genome bitmap a pipeline left on the device (pgx_bitmap_from_clusters): its token, shape, buffer
    uint64_t resident_token = 0, resident_next = 1;
    uint32_t resident_genes = 0, resident_genomes = 0;
    // the table loaded for Bernoulli likelihood evaluations (pgx_bernoulli_load*): its shape; the bitmap is a workspace slot
    uint32_t bern_genes = 0, bern_genomes = 0;
    bool bern_loaded = false;
    // of the last coordinate descent on it (pgx_bernoulli_cd*): evaluations of f, most of one solve, solves not converged, solves
    uint64_t bern_cd_stats[4] = {0, 0, 0, 0};
    // the set of keys loaded for exact look-ups (pgx_dict_load): how many, the flags they were hashed with, and the device
    // pointers of keys, offsets and table (workspace slots only dict.hip uses; valid while dict_loaded)
    bool dict_loaded = false;
    uint32_t dict_keys = 0, dict_flags = 0;
    const void *dict_d_keys = nullptr, *dict_d_offsets = nullptr, *dict_d_table = nullptr;
    // the set of patterns loaded for exact scans (pgx_pattern_load): how many, the seed and flags they were hashed with, and
    // the device pointers of blob, offsets and table + filter (workspace slots only pattern.hip uses; valid while pattern_loaded)
    bool pattern_loaded = false;
    uint32_t pattern_count = 0, pattern_seed = 0, pattern_flags = 0;
    const void *pattern_d_blob = nullptr, *pattern_d_offsets = nullptr, *pattern_d_ws = nullptr;
    // the set of patterns loaded for bounded-mismatch scans (pgx_near_load): how many, the block and flags they were hashed
    // with, the entries their table was sized for, and the device pointers of blob, offsets, max_mismatch and table + filter
    // (workspace slots only near.hip uses; valid while near_loaded)
    bool near_loaded = false;
    uint32_t near_count = 0, near_block = 0, near_flags = 0;
    uint64_t near_blocks = 0;
    const void *near_d_blob = nullptr, *near_d_offsets = nullptr, *near_d_mismatch = nullptr, *near_d_ws = nullptr;
    // of the last local alignment call (pgx_sw_pairs*): the pairs that took the pass with statistics
    uint32_t sw_stats_pairs = 0;
    // the concepts of the last formal concept decomposition (pgx_fcd*), kept for pgx_fcd_fetch: row / column indices of
    // all concepts end to end, the offsets of each concept in them (n + 1 entries), the ones left uncovered after each
    std::vector<int32_t> fcd_rows, fcd_cols;
    std::vector<uint64_t> fcd_row_off, fcd_col_off, fcd_left;
    // the library's own RCCL communicator (pgx_rccl_comm_create): the record-sharded exchange without a callback
    void *comm = nullptr;
    int comm_rank = 0, comm_world = 0;
};

// Array of n elements of T in the context's host scratch slot `slot` (uninitialised unless `fill` is given).
// A view: the memory belongs to the context and outlives the call. Check ok() after construction.
template <typename T>
struct HostVec {
    T *p = nullptr;
    size_t n = 0;
    HostVec() = default;   // bound later, by assignment
    HostVec(pgx_ctx *ctx, HostSlot slot, size_t count) { bind(ctx, slot, count); }
    HostVec(pgx_ctx *ctx, HostSlot slot, size_t count, T fill) {
        bind(ctx, slot, count);
        if (p) std::fill(p, p + n, fill);
    }
    bool ok() const { return p != nullptr || n == 0; }
    T *data() { return p; }
    const T *data() const { return p; }
    size_t size() const { return n; }
    T &operator[](size_t i) { return p[i]; }
    const T &operator[](size_t i) const { return p[i]; }
    T *begin() { return p; }
    T *end() { return p + n; }

private:
    void bind(pgx_ctx *ctx, HostSlot slot, size_t count) {
        auto &a = ctx->host_scratch[slot];
        const size_t bytes = count * sizeof(T) + 64;
        if (a.second < bytes) {
            if (a.first) (void)hipHostFree(a.first);
            a = {nullptr, 0};
            const size_t want = bytes + bytes / 4;
            void *q = nullptr;
            if (hipHostMalloc(&q, want, hipHostMallocDefault) == hipSuccess) a = {q, want};
            else (void)hipGetLastError();
        }
        p = static_cast<T *>(a.first);
        n = p ? count : 0;
        if (!p && count) n = count;  // ok() reports the failure
    }
};

// Kernels write results straight into these buffers (publish_kernel) and read lists from them, and
// the host polls for completion instead of making a synchronising call: the memory must be
// COHERENT (fine-grained, never cached by the GPU), or the device could serve a re-used list from
// its L2 and leave published records there.
constexpr unsigned kPinnedFlags = hipHostMallocCoherent | hipHostMallocMapped;
template <typename T>
struct Pinned {  // page-locked host staging buffer in a context slot: it outlives the call
    T *p = nullptr;
    size_t cap = 0;
    pgx_ctx *ctx;
    PinSlot slot;
    Pinned(pgx_ctx *c, PinSlot s) : ctx(c), slot(s) {}
    hipError_t reserve(size_t n) {
        if (n <= cap) return hipSuccess;
        auto &a = ctx->host_arena[slot];
        const size_t bytes = n * sizeof(T);
        if (!a.first || a.second < bytes) {
            if (a.first) (void)hipHostFree(a.first);
            a = {nullptr, 0};
            const size_t want = bytes + bytes / 2 + 4096;
            hipError_t e = hipHostMalloc(&a.first, want, kPinnedFlags);
            if (e != hipSuccess) return e;
            a.second = want;
        }
        p = static_cast<T *>(a.first);
        cap = a.second / sizeof(T);
        return hipSuccess;
    }
};

// RAII bracket: records start/stop events on `stream` when profiling is enabled.
struct ProfScope {
    pgx_ctx *ctx;
    hipStream_t stream;
    int slot = -1;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ProfScope(pgx_ctx *c, const char *name, hipStream_t s);
    ~ProfScope();
};

#define PGX_HIP(call)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) {                                                            \
            pgx_set_error("%s:%d: %s failed: %s", __FILE__, __LINE__, #call,               \
                          hipGetErrorString(e_));                                          \
            return PGX_ERR_HIP;                                                            \
        }                                                                                  \
    } while (0)

#define PGX_REQUIRE(cond, msg)                                                             \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            pgx_set_error("%s: %s", __func__, msg);                                        \
            return PGX_ERR_INVALID;                                                        \
        }                                                                                  \
    } while (0)

// Device buffer: a view of one slot of the context's grow-only workspace, so that repeated calls neither
// allocate nor free (hipFree of GB-sized buffers stalls the queue for milliseconds).
struct DevBuf {
    void *p = nullptr;
    pgx_ctx *ctx;
    DevSlot slot;
    DevBuf(pgx_ctx *c, DevSlot s) : ctx(c), slot(s) {}
    hipError_t alloc(size_t bytes) {
        if (!bytes) bytes = 16;
        auto &a = ctx->arena[slot];
        if (!a.first || a.second < bytes) {
            if (a.first) (void)hipFree(a.first);
            a = {nullptr, 0};
            const size_t cap = bytes + bytes / 4 + 256;
            hipError_t e = hipMalloc(&a.first, cap);
            if (e != hipSuccess) return e;
            a.second = cap;
        }
        p = a.first;
        return hipSuccess;
    }
    // The slot as an earlier call filled it (state the context keeps): never allocates or frees, and fails when the
    // slot does not hold `bytes`.
    int view(size_t bytes) {
        const auto &a = ctx->arena[slot];
        if (!a.first || a.second < bytes) {
            pgx_set_error("workspace slot %d holds %zu bytes where %zu were kept", (int)slot, a.first ? a.second : (size_t)0, bytes);
            return PGX_ERR_INTERNAL;
        }
        p = a.first;
        return PGX_OK;
    }
    template <typename T>
    T *as() {
        return static_cast<T *>(p);
    }
};

// Layout of a workspace in one allocation, by offsets alone: take() is where the part starts, `off` the size so far.
struct WsLayout : PackLayout {
    size_t take(size_t bytes) { return add(bytes).off; }
};

// Host arrays <-> the parts of ONE slot, for the host entries: an array's size is stated once, where in() / out() registers
// it; the allocation and both copies follow from that. Register every part, alloc(), upload() before the launches, download()
// after them: one hipMemcpyAsync per array in registration order, straight from / to the caller's memory, and nothing here
// synchronises. A NULL host pointer reserves a part that is never copied; neither is a part of 0 bytes.
struct DevPack {
    DevBuf buf;
    PackLayout lay;
    struct Bound { PackPart part; void *host; bool up; };
    std::vector<Bound> bound;
    DevPack(pgx_ctx *c, DevSlot s) : buf(c, s) {}
    template <typename T> PackPart in(const T *host, size_t count) { return bind(const_cast<T *>(host), count * sizeof(T), true); }
    template <typename T> PackPart out(T *host, size_t count) { return bind(host, count * sizeof(T), false); }
    hipError_t alloc() { return buf.alloc(lay.total()); }
    template <typename T> T *dev(const PackPart &part) { return reinterpret_cast<T *>(static_cast<char *>(buf.p) + part.off); }
    template <typename T> T *dev_if(const T *host, const PackPart &part) { return host ? dev<T>(part) : nullptr; }  // NULL: not wanted
    hipError_t upload(hipStream_t stream) { return copy(true, stream); }
    hipError_t download(hipStream_t stream) { return copy(false, stream); }
    // elements [first, first + count) of a part to `host`: an array of which only the device knew how much it would write
    template <typename T> hipError_t download(const PackPart &part, size_t first, size_t count, T *host, hipStream_t stream) {
        if ((first + count) * sizeof(T) > part.bytes) return hipErrorInvalidValue;
        return count ? hipMemcpyAsync(host, dev<T>(part) + first, count * sizeof(T), hipMemcpyDeviceToHost, stream) : hipSuccess;
    }

private:
    PackPart bind(void *host, size_t bytes, bool up) {
        const PackPart part = lay.add(bytes);
        if (host && bytes) bound.push_back({part, host, up});
        return part;
    }
    hipError_t copy(bool up, hipStream_t stream) {
        for (const Bound &b : bound) {
            void *d = dev<char>(b.part);
            const hipError_t e = b.up != up ? hipSuccess : hipMemcpyAsync(up ? d : b.host, up ? b.host : d, b.part.bytes,
                                                                          up ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, stream);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
};

static inline uint32_t ceil_div_u32(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

// Host-to-device copy of a large PAGEABLE buffer, enqueued on `stream`: a few threads copy 4 MB chunks into
// page-locked staging buffers of the context (two per thread) and enqueue the DMA of each chunk as soon as it is
// staged, so that the CPU copies of the threads and the DMA engine overlap. hipMemcpyAsync from pageable memory
// stages through one thread: 13.7 GB/s measured for the 370 MB of the benchmark's sequences. Small buffers
// take the plain call. Returns when every chunk has been ENQUEUED (the source may be reused; the copies complete in
// stream order).
int pgx_staged_h2d(pgx_ctx *ctx, void *dst, const void *src, size_t bytes, hipStream_t stream);

// COO records (host) -> gene x genome bitmap in d_bits, built on ctx->stream (pancore.hip). The coordinates travel
// through the workspace slots slot_rows / slot_genomes; d_bits and d_cnt are the caller's (bound to slots of its own,
// so that one user's table is not overwritten by another's call). d_cnt: 2 x u64, see presence_bitmap_kernel.
int pgx_upload_and_build_bitmap(pgx_ctx *ctx, const int32_t *rows, const int32_t *genomes, uint64_t n_records,
                                uint32_t n_rows, uint32_t n_genomes, DevSlot slot_rows, DevSlot slot_genomes, DevBuf &d_bits,
                                DevBuf &d_cnt);
// Its counterpart: the two counters back, ctx->stream synchronised; fails when a record was out of range (none of
// those was written), stores the number of duplicate coordinates through out_duplicates unless that is NULL.
int pgx_read_record_counters(pgx_ctx *ctx, DevBuf &d_cnt, uint64_t *out_duplicates);
// The two in one call, for a caller that enqueues nothing in between: the table is in d_bits, *duplicates set unless NULL.
int pgx_load_coo_bitmap(pgx_ctx *ctx, const int32_t *rows, const int32_t *genomes, uint64_t n_records, uint32_t n_rows,
                        uint32_t n_genomes, DevSlot slot_rows, DevSlot slot_genomes, DevBuf &d_bits, DevBuf &d_cnt,
                        uint64_t *duplicates);

// The bitmap pgx_bitmap_from_clusters left in the context (pancore.hip): n_genomes x stride words, n_genes rows.
struct ResidentBitmap {
    const uint64_t *d_bits;
    uint32_t n_genes, stride;
};
// Fails unless `token` names the bitmap that is resident and that has n_genomes genomes; the slot is only viewed.
int pgx_resident_bitmap(pgx_ctx *ctx, uint64_t token, uint32_t n_genomes, ResidentBitmap *out);
// d_bits = the table of G rows x S genomes gathered from it: row i, column j = row row_map[i], column col_map[j] of the
// resident bitmap (col_map NULL: the same column). The maps (host) are checked before anything else (PGX_ERR_INVALID:
// nothing was touched), then uploaded into d_map / d_cmap (NULL for a caller that never has a column map); ctx->stream is
// synchronised, so they are the caller's again on return. prof_name: the kernel's name in the profile.
int pgx_gather_resident(pgx_ctx *ctx, const ResidentBitmap &src, const int32_t *row_map, const int32_t *col_map,
                        uint32_t G, uint32_t S, DevBuf &d_map, DevBuf *d_cmap, DevBuf &d_bits,
                        const char *prof_name);

// all-gather of `count` uint64 per process with the context's RCCL communicator, enqueued on `stream` (rccl_exchange.hip)
int pgx_rccl_all_gather_u64(pgx_ctx *ctx, const void *send, void *recv, size_t count, hipStream_t stream);

// What select.hip takes from runs.hip. The rules of the run arrays (pgx.h, "Runs of allele rows"): the message of the first
// one broken or NULL -- of host arrays, and of the status word pgx_runs_check_enqueue ORs its findings into (the caller
// zeroes it first and reads it back after its launches). pgx_runs_stats_enqueue: the allele rows' counts into d_counts
// (n_alleles x int32), then total / best_allele / best_count of every run (each may be NULL), reads clamped to n_alleles.
// Both only enqueue on `stream`.
const char *pgx_runs_host_error(const uint32_t *run_start, uint32_t n_runs, const int32_t *gene_of_run, uint32_t n_alleles,
                                uint32_t n_genes);
const char *pgx_runs_status_error(uint32_t status);
// The host entries' common start: the record and run arrays checked (messages under the name `who`), both tables built (the
// gene table only with gene_of_run), their counters read back -- ctx->stream is synchronised -- and reported through
// out_duplicates (2 x u64 unless NULL), run_start / gene_of_run enqueued. `nothing`: duplicates or no runs, the caller returns.
struct RunsLoaded {
    const uint64_t *d_abits, *d_gbits;          // d_gbits and d_gene_of_run: NULL without gene_of_run
    const uint32_t *d_run_start;
    const int32_t *d_gene_of_run;
    bool nothing;
};
int pgx_runs_load_host(pgx_ctx *ctx, const char *who, const int32_t *a_rows, const int32_t *a_genomes, uint64_t a_records,
                       uint32_t n_alleles, const int32_t *g_rows, const int32_t *g_genomes, uint64_t g_records, uint32_t n_genes,
                       uint32_t n_genomes, const uint32_t *run_start, uint32_t n_runs, const int32_t *gene_of_run,
                       uint64_t *out_duplicates, RunsLoaded *out);
int pgx_runs_check_enqueue(pgx_ctx *ctx, const uint32_t *d_run_start, const int32_t *d_gene_of_run, uint32_t n_runs,
                           uint32_t n_alleles, uint32_t n_genes, uint32_t *d_status, hipStream_t stream);
int pgx_runs_stats_enqueue(pgx_ctx *ctx, const uint64_t *d_abits, uint32_t n_alleles, uint32_t n_genomes,
                           const uint32_t *d_run_start, uint32_t n_runs, int32_t *d_counts, uint64_t *d_total,
                           int32_t *d_best_allele, uint32_t *d_best_count, hipStream_t stream);
