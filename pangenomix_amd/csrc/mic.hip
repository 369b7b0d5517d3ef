// The two device steps of amr_inference (reference amr_inference.py: extract_primary_stnds and extract_mic_calls count
// distinct tuples with value_counts / collections.Counter, infer_sir is a scalar function called once per row).
//
// tuple_group: n records of k int32 columns, column-major (cols[c * n + i]).
//   first[i] = the smallest j whose record equals record i, count[i] = how many records equal record i when first[i] == i and
//   0 otherwise, *n_distinct = the number of i with first[i] == i. All three are functions of the input alone: `first` is a
//   minimum over a set (atomicMin), `count` an integer sum (atomicAdd); no atomic decides an order. Hashes only say where to
//   look: a slot is shared only after all k columns have been compared.
//   tg_build_kernel: one lane per record, columns read coalesced. The lanes of a wave that hold the same record combine
//     first -- the lowest lane of each set of equal records leads (its index is the set's smallest) -- so a record every lane
//     holds costs the wave one probe and two atomics, not 64. A leader walks the open-addressing table from its hash: an
//     empty slot is claimed with a CAS of its index; a taken slot holds the index of SOME record of its tuple (atomicMin only
//     ever replaces it by another of the same tuple), which is compared column by column. The leader then lowers the slot to
//     its index, adds its set's size to the slot's counter and hands the slot's number to its lanes (slot_of[i]).
//   tg_read_kernel (the kernel boundary gives the visibility): first[i] = table[slot_of[i]], count[i], and one integer
//     atomicAdd per wave for n_distinct.
//
// mic_infer: one lane per row over structure-of-arrays inputs, the body of infer_sir (pgx.h "SIR inference"); the case tables
//   are small and shared, the sorted runs are searched in global memory. One plain launch, no atomics.
// Every index read from an offset array is clamped to the array it points into, so the device entries touch nothing outside
// the caller's buffers whatever the offsets hold.
#include "pgx_internal.h"

namespace {

typedef unsigned long long u64;

constexpr int MC_THREADS = 256;
constexpr uint32_t MC_MAX_GRID = 4096;
constexpr uint32_t TG_MAX_N = 1u << 24, TG_MAX_K = PGX_TUPLE_MAX_COLUMNS;
constexpr uint32_t TG_EMPTY = 0xFFFFFFFFu;
constexpr uint32_t MI_MAX_TABLE = 1u << 24;

// ---- tuple_group ------------------------------------------------------------------------------------------------------------
uint32_t tg_slots(uint32_t n) {
    uint32_t slots = 64;
    while (slots < 2 * n) slots <<= 1;                     // (n < 2^24: at most 2^25)
    return slots;
}

struct TgWs {
    size_t table, counts, slot_of, bytes;
};

TgWs tg_layout(uint32_t n) {
    TgWs g;
    WsLayout lay;
    g.table = lay.take((size_t)tg_slots(n) * 4);
    g.counts = lay.take((size_t)tg_slots(n) * 4);
    g.slot_of = lay.take((size_t)n * 4);
    g.bytes = lay.off;
    return g;
}

__device__ __forceinline__ u64 tg_mix(u64 h) {
    h ^= h >> 33;
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33;
    h *= 0xC4CEB9FE1A85EC53ull;
    h ^= h >> 33;
    return h;
}

template <uint32_t K>
__global__ __launch_bounds__(MC_THREADS) void tg_build_kernel(const int32_t *__restrict__ cols, uint32_t n, uint32_t flags,
                                                             uint32_t *table, uint32_t *counts, uint32_t mask,
                                                             uint32_t *__restrict__ slot_of) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_rounds = (n + MC_THREADS - 1u) / MC_THREADS;
    // every lane takes the same rounds, so the cross-lane reads below are made by whole waves
    for (uint32_t round = blockIdx.x; round < n_rounds; round += gridDim.x) {
        const uint32_t i = round * MC_THREADS + threadIdx.x;
        const bool live = i < n;
        int32_t v[K];
        u64 h = 0x9E3779B97F4A7C15ull;
        for (uint32_t c = 0; c < K; ++c) {
            v[c] = live ? cols[(size_t)c * n + i] : 0;
            h = tg_mix(h ^ (u64)(uint32_t)v[c]);
        }
        if (flags & PGX_TUPLE_NARROW_HASH) h &= 7ull;
        // the sets of equal records of this wave: the lowest lane not yet in a set leads the next one
        u64 todo = __ballot(live);
        uint32_t leader = lane, members = 0;
        while (todo != 0ull) {
            const uint32_t l = (uint32_t)__ffsll((long long)todo) - 1u;
            bool same = live;
            for (uint32_t c = 0; c < K; ++c) same = same && __shfl(v[c], (int)l, 64) == v[c];
            const u64 set = __ballot(same) & todo;         // (lane l itself is in it)
            if (same) {
                leader = l;
                members = (uint32_t)__popcll(set);
            }
            todo &= ~set;
        }
        uint32_t s = 0;
        if (live && leader == lane) {
            s = (uint32_t)h & mask;
            // `mask + 1` >= 2 n slots, of which at most n are taken: an empty one is always met
            for (;;) {
                uint32_t e = __atomic_load_n(&table[s], __ATOMIC_RELAXED);
                if (e == TG_EMPTY) {
                    e = atomicCAS(&table[s], TG_EMPTY, i);
                    if (e == TG_EMPTY) break;              // claimed: the slot holds i
                }
                e = e < n ? e : i;                         // (a slot only ever holds an index below n)
                bool equal = true;
                for (uint32_t c = 0; c < K; ++c) equal = equal && cols[(size_t)c * n + e] == v[c];
                if (equal) {
                    atomicMin(&table[s], i);               // (a minimum: any order)
                    break;
                }
                s = (s + 1u) & mask;
            }
            atomicAdd(&counts[s], members);                // (a sum: any order)
        }
        s = (uint32_t)__shfl((int)s, (int)leader, 64);
        if (live) slot_of[i] = s;
    }
}

__global__ __launch_bounds__(MC_THREADS) void tg_read_kernel(const uint32_t *__restrict__ table,
                                                            const uint32_t *__restrict__ counts,
                                                            const uint32_t *__restrict__ slot_of, uint32_t n, uint32_t mask,
                                                            int32_t *__restrict__ first, uint32_t *__restrict__ count,
                                                            uint32_t *n_distinct) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_rounds = (n + MC_THREADS - 1u) / MC_THREADS;
    uint32_t mine = 0;
    for (uint32_t round = blockIdx.x; round < n_rounds; round += gridDim.x) {
        const uint32_t i = round * MC_THREADS + threadIdx.x;
        if (i < n) {
            const uint32_t s = slot_of[i] & mask;
            const uint32_t f = table[s];
            first[i] = (int32_t)f;
            count[i] = f == i ? counts[s] : 0u;
            mine += f == i ? 1u : 0u;
        }
    }
    for (int d = 32; d >= 1; d >>= 1) mine += (uint32_t)__shfl_down((int)mine, d, 64);
    if (lane == 0u && mine) atomicAdd(n_distinct, mine);   // (a sum: any order)
}

int tg_sizes(pgx_ctx *ctx, uint32_t n, uint32_t k, uint32_t flags) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(k >= 1 && k <= TG_MAX_K, "k must lie in 1..PGX_TUPLE_MAX_COLUMNS");
    PGX_REQUIRE(n < TG_MAX_N, "n must be below 2^24");
    PGX_REQUIRE((flags & ~PGX_TUPLE_NARROW_HASH) == 0, "unknown flags");
    return PGX_OK;
}

template <uint32_t K>
void tg_build(uint32_t grid, hipStream_t stream, const int32_t *d_cols, uint32_t n, uint32_t flags, uint32_t *table,
              uint32_t *counts, uint32_t mask, uint32_t *slot_of) {
    tg_build_kernel<K><<<grid, MC_THREADS, 0, stream>>>(d_cols, n, flags, table, counts, mask, slot_of);
}

// Only enqueues. n >= 1.
int tg_launch(pgx_ctx *ctx, const int32_t *d_cols, uint32_t n, uint32_t k, uint32_t flags, int32_t *d_first, uint32_t *d_count,
              uint32_t *d_distinct, uint8_t *ws, hipStream_t stream) {
    const TgWs g = tg_layout(n);
    uint32_t *table = (uint32_t *)(ws + g.table), *counts = (uint32_t *)(ws + g.counts), *slot_of = (uint32_t *)(ws + g.slot_of);
    const uint32_t slots = tg_slots(n), mask = slots - 1u;
    const uint32_t blocks = ceil_div_u32(n, MC_THREADS), grid = blocks < MC_MAX_GRID ? blocks : MC_MAX_GRID;
    PGX_HIP(hipMemsetAsync(table, 0xFF, (size_t)slots * 4, stream));
    PGX_HIP(hipMemsetAsync(counts, 0, (size_t)slots * 4, stream));
    PGX_HIP(hipMemsetAsync(d_distinct, 0, 4, stream));
    {
        ProfScope prof(ctx, "tg_build_kernel", stream);
        switch (k) {
        case 1: tg_build<1>(grid, stream, d_cols, n, flags, table, counts, mask, slot_of); break;
        case 2: tg_build<2>(grid, stream, d_cols, n, flags, table, counts, mask, slot_of); break;
        case 3: tg_build<3>(grid, stream, d_cols, n, flags, table, counts, mask, slot_of); break;
        case 4: tg_build<4>(grid, stream, d_cols, n, flags, table, counts, mask, slot_of); break;
        case 5: tg_build<5>(grid, stream, d_cols, n, flags, table, counts, mask, slot_of); break;
        case 6: tg_build<6>(grid, stream, d_cols, n, flags, table, counts, mask, slot_of); break;
        case 7: tg_build<7>(grid, stream, d_cols, n, flags, table, counts, mask, slot_of); break;
        default: tg_build<8>(grid, stream, d_cols, n, flags, table, counts, mask, slot_of); break;
        }
    }
    {
        ProfScope prof(ctx, "tg_read_kernel", stream);
        tg_read_kernel<<<grid, MC_THREADS, 0, stream>>>(table, counts, slot_of, n, mask, d_first, d_count, d_distinct);
    }
    PGX_HIP(hipGetLastError());
    return PGX_OK;
}

int tg_dev(pgx_ctx *ctx, const int32_t *d_cols, uint32_t n, uint32_t k, uint32_t flags, int32_t *d_first, uint32_t *d_count,
           uint32_t *d_distinct, void *d_ws, size_t ws_bytes, hipStream_t stream) {
    int rc = tg_sizes(ctx, n, k, flags);
    if (rc != PGX_OK) return rc;
    PGX_REQUIRE(d_distinct, "NULL n_distinct");
    PGX_REQUIRE(((uintptr_t)d_distinct & 3u) == 0, "n_distinct must be 4-byte aligned");
    if (n == 0) {
        PGX_HIP(hipMemsetAsync(d_distinct, 0, 4, stream));
        PGX_HIP(hipStreamSynchronize(stream));
        return PGX_OK;
    }
    PGX_REQUIRE(d_cols && d_first && d_count, "NULL argument");
    PGX_REQUIRE(d_ws && ws_bytes >= tg_layout(n).bytes, "workspace too small (see pgx_tuple_group_workspace_bytes)");
    PGX_REQUIRE(((uintptr_t)d_ws & 15u) == 0, "workspace must be 16-byte aligned");
    PGX_REQUIRE((((uintptr_t)d_cols | (uintptr_t)d_first | (uintptr_t)d_count) & 3u) == 0,
                "cols, first and count must be 4-byte aligned");
    rc = tg_launch(ctx, d_cols, n, k, flags, d_first, d_count, d_distinct, (uint8_t *)d_ws, stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(hipStreamSynchronize(stream));
    return PGX_OK;
}

int tg_host(pgx_ctx *ctx, const int32_t *cols, uint32_t n, uint32_t k, uint32_t flags, int32_t *out_first, uint32_t *out_count,
            uint32_t *out_distinct) {
    int rc = tg_sizes(ctx, n, k, flags);
    if (rc != PGX_OK) return rc;
    PGX_REQUIRE(out_distinct, "NULL n_distinct");
    if (n == 0) {
        *out_distinct = 0;
        return PGX_OK;
    }
    PGX_REQUIRE(cols && out_first && out_count, "NULL argument");
    PGX_HIP(hipSetDevice(ctx->device_id));
    DevBuf d_ws(ctx, TG_SLOT_WS);
    DevPack in(ctx, TG_SLOT_IN), res(ctx, TG_SLOT_OUT);
    const PackPart i_cols = in.in(cols, (size_t)n * k);
    const PackPart r_first = res.out(out_first, n), r_count = res.out(out_count, n), r_distinct = res.out(out_distinct, 1);
    PGX_HIP(in.alloc());
    PGX_HIP(res.alloc());
    PGX_HIP(d_ws.alloc(tg_layout(n).bytes));
    PGX_HIP(in.upload(ctx->stream));
    rc = tg_launch(ctx, in.dev<int32_t>(i_cols), n, k, flags, res.dev<int32_t>(r_first), res.dev<uint32_t>(r_count),
                   res.dev<uint32_t>(r_distinct), d_ws.as<uint8_t>(), ctx->stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(res.download(ctx->stream));
    PGX_HIP(hipStreamSynchronize(ctx->stream));
    return PGX_OK;
}

// ---- mic_infer --------------------------------------------------------------------------------------------------------------
struct MicTables {
    const uint32_t *class_begin;
    const int32_t *sir;
    const uint8_t *role;
    const uint32_t *fl_begin, *tk_begin;
    const double *fvals;
    const int32_t *tvals;
    uint32_t n_cases, n_entries, n_fvals, n_tvals;
};

struct MicRows {
    const int32_t *row_case;
    const uint8_t *sign, *combo, *kind;
    const int32_t *token;
    const double *value;
};

__device__ __forceinline__ uint32_t clamp_u32(uint32_t x, uint32_t hi) { return x < hi ? x : hi; }

// is x an element of the sorted run a[b .. e)? A lower bound, then one == (on doubles: a NaN is no member)
template <typename T>
__device__ __forceinline__ bool in_sorted_run(const T *__restrict__ a, uint32_t b, uint32_t e, T x) {
    const uint32_t end = e;
    while (b < e) {
        const uint32_t m = b + ((e - b) >> 1);
        if (a[m] < x) b = m + 1u;
        else e = m;
    }
    return b < end && a[b] == x;
}

// 0: class entry e does not take the row, 1: it does, 2: the host has to decide
__device__ __forceinline__ int mic_try(const MicTables &t, uint32_t e, bool combo, uint32_t kind, int32_t token, double v) {
    const uint32_t fb = clamp_u32(t.fl_begin[e], t.n_fvals), fe = clamp_u32(t.fl_begin[e + 1], t.n_fvals);
    const uint32_t tb = clamp_u32(t.tk_begin[e], t.n_tvals), te = clamp_u32(t.tk_begin[e + 1], t.n_tvals);
    if (kind == 1u ? in_sorted_run(t.fvals, fb, fe, v) : (token >= 0 && in_sorted_run(t.tvals, tb, te, token))) return 1;
    if (combo) return 0;
    if (te > tb || fe <= fb) return 2;                     // min() / max() over a string MIC, or over nothing
    const uint32_t role = t.role[e];
    const double lo = t.fvals[fb], hi = t.fvals[fe - 1u];
    return (role == 0u || v >= lo) && (role == 1u || v <= hi) ? 1 : 0;
}

__global__ __launch_bounds__(MC_THREADS) void mic_infer_kernel(MicTables t, MicRows r, uint32_t n, int32_t *__restrict__ out) {
    const uint32_t n_rounds = (n + MC_THREADS - 1u) / MC_THREADS;
    for (uint32_t round = blockIdx.x; round < n_rounds; round += gridDim.x) {
        const uint32_t i = round * MC_THREADS + threadIdx.x;
        if (i >= n) continue;
        const int32_t c = r.row_case[i];
        const uint32_t sign = r.sign[i];
        int32_t res = -1;
        if (c >= 0 && (uint32_t)c < t.n_cases && sign < 3u) {
            const uint32_t eb = clamp_u32(t.class_begin[c], t.n_entries), ee = clamp_u32(t.class_begin[c + 1], t.n_entries);
            const bool combo = r.combo[i] != 0;
            const uint32_t kind = r.kind[i];
            const int32_t token = r.token[i];
            const double v = (!combo || kind == 1u) ? r.value[i] : 0.0;
            for (uint32_t e = eb; e < ee; ++e) {
                // an inequality is tried on the case's 'susceptible' ('<', '<=') or 'resistant' ('>', '>=') entry alone
                if (sign != 0u && t.role[e] != sign - 1u) continue;
                const int hit = mic_try(t, e, combo, kind, token, v);
                if (hit) {
                    res = hit == 1 ? t.sir[e] : -2;
                    break;
                }
                if (sign != 0u) break;                     // (a case names a class once)
            }
        }
        out[i] = res;
    }
}

int mic_sizes(pgx_ctx *ctx, uint32_t n_cases, uint32_t n_entries, uint32_t n_fvals, uint32_t n_tvals, uint64_t n) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(n < (1ull << 31), "n must be below 2^31");
    PGX_REQUIRE(n_cases < MI_MAX_TABLE && n_entries < MI_MAX_TABLE && n_fvals < MI_MAX_TABLE && n_tvals < MI_MAX_TABLE,
                "cases, class entries and list elements must each be fewer than 2^24");
    return PGX_OK;
}

int mic_launch(pgx_ctx *ctx, const MicTables &t, const MicRows &r, uint32_t n, int32_t *d_out, hipStream_t stream) {
    const uint32_t blocks = ceil_div_u32(n, MC_THREADS);
    {
        ProfScope prof(ctx, "mic_infer_kernel", stream);
        mic_infer_kernel<<<blocks < MC_MAX_GRID ? blocks : MC_MAX_GRID, MC_THREADS, 0, stream>>>(t, r, n, d_out);
    }
    PGX_HIP(hipGetLastError());
    return PGX_OK;
}

int mic_dev(pgx_ctx *ctx, const MicTables &t, const MicRows &r, uint64_t n, int32_t *d_out, hipStream_t stream) {
    int rc = mic_sizes(ctx, t.n_cases, t.n_entries, t.n_fvals, t.n_tvals, n);
    if (rc != PGX_OK) return rc;
    if (n == 0) return PGX_OK;
    PGX_REQUIRE(t.class_begin && t.fl_begin && t.tk_begin && r.row_case && r.sign && r.combo && r.kind && r.token && r.value && d_out,
                "NULL argument");
    PGX_REQUIRE((t.n_entries == 0 || (t.sir && t.role)) && (t.n_fvals == 0 || t.fvals) && (t.n_tvals == 0 || t.tvals),
                "NULL table");
    PGX_REQUIRE((((uintptr_t)t.fvals | (uintptr_t)r.value) & 7u) == 0, "fvals and value must be 8-byte aligned");
    PGX_REQUIRE((((uintptr_t)t.class_begin | (uintptr_t)t.sir | (uintptr_t)t.fl_begin | (uintptr_t)t.tk_begin | (uintptr_t)t.tvals |
                  (uintptr_t)r.row_case | (uintptr_t)r.token | (uintptr_t)d_out) & 3u) == 0,
                "the 32-bit arrays must be 4-byte aligned");
    rc = mic_launch(ctx, t, r, (uint32_t)n, d_out, stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(hipStreamSynchronize(stream));
    return PGX_OK;
}

int mic_host(pgx_ctx *ctx, const MicTables &t, const MicRows &r, uint64_t n64, int32_t *out) {
    int rc = mic_sizes(ctx, t.n_cases, t.n_entries, t.n_fvals, t.n_tvals, n64);
    if (rc != PGX_OK) return rc;
    const uint32_t n = (uint32_t)n64;
    PGX_REQUIRE(t.class_begin && t.fl_begin && t.tk_begin, "NULL offsets");
    PGX_REQUIRE(t.class_begin[0] == 0 && t.fl_begin[0] == 0 && t.tk_begin[0] == 0, "offsets must start at 0");
    for (uint32_t c = 0; c < t.n_cases; ++c) PGX_REQUIRE(t.class_begin[c] <= t.class_begin[c + 1], "offsets must not decrease");
    PGX_REQUIRE(t.class_begin[t.n_cases] == t.n_entries, "class_begin must end at n_entries");
    PGX_REQUIRE(t.n_entries == 0 || (t.sir && t.role), "NULL sir or role");
    for (uint32_t e = 0; e < t.n_entries; ++e) {
        PGX_REQUIRE(t.fl_begin[e] <= t.fl_begin[e + 1] && t.tk_begin[e] <= t.tk_begin[e + 1], "offsets must not decrease");
        PGX_REQUIRE(t.role[e] <= 2 && t.sir[e] >= 0, "a role must be 0, 1 or 2 and a sir code at least 0");
    }
    PGX_REQUIRE(t.fl_begin[t.n_entries] == t.n_fvals && t.tk_begin[t.n_entries] == t.n_tvals,
                "fl_begin and tk_begin must end at n_fvals and n_tvals");
    PGX_REQUIRE((t.n_fvals == 0 || t.fvals) && (t.n_tvals == 0 || t.tvals), "NULL fvals or tvals");
    for (uint32_t e = 0; e < t.n_entries; ++e) {           // sorted runs (a NaN is refused: it is in no order)
        for (uint32_t j = t.fl_begin[e]; j + 1 < t.fl_begin[e + 1]; ++j)
            PGX_REQUIRE(t.fvals[j] <= t.fvals[j + 1], "a run of fvals must be sorted and hold no NaN");
        if (t.fl_begin[e + 1] > t.fl_begin[e])
            PGX_REQUIRE(t.fvals[t.fl_begin[e + 1] - 1] == t.fvals[t.fl_begin[e + 1] - 1], "a run of fvals must hold no NaN");
        for (uint32_t j = t.tk_begin[e]; j + 1 < t.tk_begin[e + 1]; ++j)
            PGX_REQUIRE(t.tvals[j] <= t.tvals[j + 1], "a run of tvals must be sorted");
    }
    if (n == 0) return PGX_OK;
    PGX_REQUIRE(r.row_case && r.sign && r.combo && r.kind && r.token && r.value && out, "NULL argument");
    PGX_HIP(hipSetDevice(ctx->device_id));
    DevPack tab(ctx, MI_SLOT_TABLES), rows(ctx, MI_SLOT_ROWS), res(ctx, MI_SLOT_OUT);
    const PackPart p_cb = tab.in(t.class_begin, (size_t)t.n_cases + 1), p_sir = tab.in(t.sir, t.n_entries),
                   p_role = tab.in(t.role, t.n_entries), p_fb = tab.in(t.fl_begin, (size_t)t.n_entries + 1),
                   p_tb = tab.in(t.tk_begin, (size_t)t.n_entries + 1), p_fv = tab.in(t.fvals, t.n_fvals),
                   p_tv = tab.in(t.tvals, t.n_tvals);
    const PackPart p_case = rows.in(r.row_case, n), p_sign = rows.in(r.sign, n), p_combo = rows.in(r.combo, n),
                   p_kind = rows.in(r.kind, n), p_token = rows.in(r.token, n), p_value = rows.in(r.value, n);
    const PackPart r_out = res.out(out, n);
    PGX_HIP(tab.alloc());
    PGX_HIP(rows.alloc());
    PGX_HIP(res.alloc());
    PGX_HIP(tab.upload(ctx->stream));
    PGX_HIP(rows.upload(ctx->stream));
    MicTables dt = t;
    dt.class_begin = tab.dev<uint32_t>(p_cb);
    dt.sir = tab.dev<int32_t>(p_sir);
    dt.role = tab.dev<uint8_t>(p_role);
    dt.fl_begin = tab.dev<uint32_t>(p_fb);
    dt.tk_begin = tab.dev<uint32_t>(p_tb);
    dt.fvals = tab.dev<double>(p_fv);
    dt.tvals = tab.dev<int32_t>(p_tv);
    const MicRows dr = {rows.dev<int32_t>(p_case), rows.dev<uint8_t>(p_sign),  rows.dev<uint8_t>(p_combo),
                        rows.dev<uint8_t>(p_kind), rows.dev<int32_t>(p_token), rows.dev<double>(p_value)};
    rc = mic_launch(ctx, dt, dr, n, res.dev<int32_t>(r_out), ctx->stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(res.download(ctx->stream));
    PGX_HIP(hipStreamSynchronize(ctx->stream));
    return PGX_OK;
}

}  // namespace

extern "C" {

size_t pgx_tuple_group_workspace_bytes(uint32_t n, uint32_t k) {
    if (n >= TG_MAX_N || k < 1 || k > TG_MAX_K) return 0;
    return tg_layout(n).bytes;
}

int pgx_tuple_group(pgx_ctx *ctx, const int32_t *cols, uint32_t n, uint32_t k, uint32_t flags, int32_t *out_first,
                    uint32_t *out_count, uint32_t *out_n_distinct) {
    return guarded(__func__, [&] { return tg_host(ctx, cols, n, k, flags, out_first, out_count, out_n_distinct); });
}

int pgx_tuple_group_dev(pgx_ctx *ctx, const int32_t *d_cols, uint32_t n, uint32_t k, uint32_t flags, int32_t *d_first,
                        uint32_t *d_count, uint32_t *d_n_distinct, void *d_workspace, size_t workspace_bytes, void *stream) {
    return guarded(__func__, [&] {
        return tg_dev(ctx, d_cols, n, k, flags, d_first, d_count, d_n_distinct, d_workspace, workspace_bytes, (hipStream_t)stream);
    });
}

int pgx_mic_infer(pgx_ctx *ctx, const uint32_t *class_begin, uint32_t n_cases, const int32_t *sir, const uint8_t *role,
                  const uint32_t *fl_begin, const uint32_t *tk_begin, uint32_t n_entries, const double *fvals, uint32_t n_fvals,
                  const int32_t *tvals, uint32_t n_tvals, const int32_t *row_case, const uint8_t *sign, const uint8_t *combo,
                  const uint8_t *kind, const int32_t *token, const double *value, uint64_t n, int32_t *out) {
    return guarded(__func__, [&] {
        const MicTables t = {class_begin, sir, role, fl_begin, tk_begin, fvals, tvals, n_cases, n_entries, n_fvals, n_tvals};
        const MicRows r = {row_case, sign, combo, kind, token, value};
        return mic_host(ctx, t, r, n, out);
    });
}

int pgx_mic_infer_dev(pgx_ctx *ctx, const uint32_t *d_class_begin, uint32_t n_cases, const int32_t *d_sir, const uint8_t *d_role,
                      const uint32_t *d_fl_begin, const uint32_t *d_tk_begin, uint32_t n_entries, const double *d_fvals,
                      uint32_t n_fvals, const int32_t *d_tvals, uint32_t n_tvals, const int32_t *d_case, const uint8_t *d_sign,
                      const uint8_t *d_combo, const uint8_t *d_kind, const int32_t *d_token, const double *d_value, uint64_t n,
                      int32_t *d_out, void *stream) {
    return guarded(__func__, [&] {
        const MicTables t = {d_class_begin, d_sir, d_role, d_fl_begin, d_tk_begin, d_fvals, d_tvals,
                             n_cases,       n_entries, n_fvals, n_tvals};
        const MicRows r = {d_case, d_sign, d_combo, d_kind, d_token, d_value};
        return mic_dev(ctx, t, r, n, d_out, (hipStream_t)stream);
    });
}

}  // extern "C"
