// Ordered de-duplication of rows of integer ids and the plurality vote of runs of rows (reference pangenome.py:1702-1810
// extract_annotations: one OrderedDict.fromkeys per names line and one collections.Counter per gene). Ids are ids: what an id
// stands for -- an annotation string, a protein id nobody annotated -- is the caller's business. pgx.h has the definitions.
//
// A row's list L(r) is its ids without the repeats, in order. Its 64-bit hash is the wrapping sum, over the kept ids, of
// mix(id, place in the list), finished with the list's length: a sum has no order, so lanes add their ids in any order and
// an id's place still counts. The hash only decides WHERE to look: two lists are called equal after their lengths and every
// element have been compared, so the result is exact whatever the hash does -- PGX_ANNOT_NARROW_HASH keeps 3 bits of every
// hash (of a list, and of an id in the long-row set) and must give the same output.
//
// Kernels (plain launches on one stream):
//   annot_rows_kernel        a group of AN_GROUP lanes owns one row of at most AN_ROW_TILE ids: every lane compares its ids
//                            with the ones before them, a ballot of the group gives every kept id its place; writes keep,
//                            the list (ktok, at the row's own offset), its hash and its length
//   annot_long_rows_kernel   one wave owns a longer row: a set in LDS (open addressing on the id) holds each id's smallest
//                            position -- atomicMin, a minimum has no order. The set takes AN_SET_FILL ids; a row with more
//                            distinct ids takes another round over the positions the round before could not place (marked 2
//                            in keep meanwhile), so a row of any length is handled and every id is decided by the one round
//                            that held it.
//   annot_short_runs_kernel  one wave owns a run of at most AN_RUN_TILE rows, lane = row: rep = the smallest row of the run
//                            with an equal list (candidates by shuffled hash and length, then the exact compare), count =
//                            the lanes with the same rep, winner = the largest (count, -lane) of the wave
//   annot_long_runs_kernel   one workgroup owns a longer run. Its table is the run's own rows' slots of three arrays in the
//                            workspace (as many slots as rows, so a run of any size fits and no two runs share a slot): a
//                            list is looked up from its hash, an entry names a row with that list (CAS on an empty slot:
//                            WHICH equal row gets there first decides nothing, all of them hold the same list), and the
//                            class's smallest row and size are an atomicMin and an atomicAdd. Then the largest
//                            (size, -smallest row) of the table, and every row against its class's smallest row.
// The table of the long runs lies in global memory rather than LDS: one path for every run size, and only the workgroup
// that owns the run touches it, through atomics.
#include "pgx_internal.h"
#include "string_hash.h"

namespace {

using string_hash::fmix;
using string_hash::u64;

constexpr int AN_THREADS = 256;
constexpr uint32_t AN_WAVES = AN_THREADS / 64;
constexpr uint32_t AN_GROUP = 16;                           // lanes per short row
constexpr uint32_t AN_ROW_STEPS = 4;
constexpr uint32_t AN_ROW_TILE = AN_GROUP * AN_ROW_STEPS;   // ids of a row a lane group handles (pgx_annot_row_tile)
constexpr uint32_t AN_GROUPS_PER_BLOCK = AN_THREADS / AN_GROUP;
constexpr uint32_t AN_RUN_TILE = 64;                        // rows of a run one wave handles (pgx_annot_run_tile)
constexpr uint32_t AN_SET_SLOTS = 2048;                     // the long-row set: ids and positions, 16 KiB of LDS
constexpr uint32_t AN_SET_FILL = AN_SET_SLOTS / 2;
constexpr uint32_t AN_MAX_GRID = 8192;
constexpr uint32_t AN_MAX_ROWS = 1u << 24;
constexpr u64 AN_MAX_TOKENS = 1ull << 31;
constexpr uint32_t AN_EMPTY = ~0u;
constexpr uint32_t AN_NO_REP = 64;
static_assert(AN_RUN_TILE == 64, "lane = row");
static_assert(AN_SET_FILL > 64, "a step of 64 insertions fits behind the fill mark");

__device__ __forceinline__ u64 id_mix(int32_t id, uint32_t place) {
    return fmix(((u64)(uint32_t)id + 1ull) * 0x9E3779B97F4A7C15ull ^ ((u64)place + 1ull) * 0xC2B2AE3D27D4EB4Full);
}

__device__ __forceinline__ u64 list_hash(u64 sum, uint32_t klen, uint32_t flags) {
    const u64 h = fmix(sum + (u64)klen * 0xD6E8FEB86659FD93ull + 0x2545F4914F6CDD1Dull);
    return (flags & PGX_ANNOT_NARROW_HASH) ? (h & 7ull) : h;
}

// [begin, begin + len) of row r, clamped into [0, n_tokens) whatever the offsets hold (the host entry has checked them; a
// device caller's are trusted for the result, not for memory safety). n_tokens < 2^31.
__device__ __forceinline__ void row_span(const u64 *__restrict__ row_off, uint32_t r, u64 n_tokens, u64 &begin, uint32_t &len) {
    u64 b = row_off[r], e = row_off[r + 1];
    b = b < n_tokens ? b : n_tokens;
    e = e < n_tokens ? e : n_tokens;
    begin = b;
    len = e > b ? (uint32_t)(e - b) : 0u;
}

__device__ __forceinline__ void run_span(const uint32_t *__restrict__ run_off, uint32_t u, uint32_t n_rows, uint32_t &start,
                                         uint32_t &size) {
    uint32_t b = run_off[u], e = run_off[u + 1];
    b = b < n_rows ? b : n_rows;
    e = e < n_rows ? e : n_rows;
    start = b;
    size = e > b ? e - b : 0u;
}

__device__ __forceinline__ u64 shfl_u64(u64 v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
    return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ bool lists_equal(const int32_t *__restrict__ ktok, u64 a, u64 b, uint32_t klen) {
    for (uint32_t i = 0; i < klen; ++i)
        if (ktok[a + i] != ktok[b + i]) return false;
    return true;
}

// ---- rows -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AN_THREADS) void annot_rows_kernel(const int32_t *__restrict__ tok,
                                                                const u64 *__restrict__ row_off, uint32_t n_rows,
                                                                u64 n_tokens, uint32_t flags, uint8_t *__restrict__ keep,
                                                                int32_t *__restrict__ ktok, u64 *__restrict__ row_hash,
                                                                uint32_t *__restrict__ row_klen) {
    const uint32_t sub = threadIdx.x & (AN_GROUP - 1u), lane = threadIdx.x & 63u;
    const uint32_t shift = lane & ~(AN_GROUP - 1u);
    const uint32_t below = (1u << sub) - 1u;
    const uint32_t n_rounds = (n_rows + AN_GROUPS_PER_BLOCK - 1u) / AN_GROUPS_PER_BLOCK;
    // every lane takes the same rounds and the same steps (a group without a short row works on the empty row), so the
    // ballots and shuffles are reached by whole waves
    for (uint32_t round = blockIdx.x; round < n_rounds; round += gridDim.x) {
        const uint32_t r = round * AN_GROUPS_PER_BLOCK + threadIdx.x / AN_GROUP;
        u64 b = 0;
        uint32_t len = 0;
        if (r < n_rows) row_span(row_off, r, n_tokens, b, len);
        const bool mine = r < n_rows && len <= AN_ROW_TILE;
        if (!mine) len = 0;
        uint32_t klen = 0;
        u64 sum = 0;
        for (uint32_t step = 0; step < AN_ROW_STEPS; ++step) {
            const uint32_t p = step * AN_GROUP + sub;
            const bool valid = p < len;
            int32_t id = 0;
            bool kept = false;
            if (valid) {
                id = tok[b + p];
                kept = true;
                for (uint32_t q = 0; q < p; ++q)
                    if (tok[b + q] == id) { kept = false; break; }
            }
            const uint32_t bits = (uint32_t)(__ballot(kept) >> shift) & 0xFFFFu;
            const uint32_t place = klen + (uint32_t)__popc(bits & below);
            if (valid) {
                keep[b + p] = kept ? 1 : 0;
                if (kept) {
                    ktok[b + place] = id;                   // place <= p: inside the row
                    sum += id_mix(id, place);
                }
            }
            klen += (uint32_t)__popc(bits);
        }
        for (uint32_t d = AN_GROUP / 2; d >= 1; d >>= 1) {
            const uint32_t lo = __shfl_xor((int)(uint32_t)sum, (int)d, (int)AN_GROUP);
            const uint32_t hi = __shfl_xor((int)(uint32_t)(sum >> 32), (int)d, (int)AN_GROUP);
            sum += ((u64)hi << 32) | lo;
        }
        if (mine && sub == 0u) {
            row_hash[r] = list_hash(sum, klen, flags);
            row_klen[r] = klen;
        }
    }
}

// One wave (the whole workgroup), one row of more than AN_ROW_TILE ids.
__device__ void long_row(const int32_t *__restrict__ tok, u64 b, uint32_t len, uint32_t flags, uint8_t *keep,
                         int32_t *__restrict__ ktok, int32_t *s_id, uint32_t *s_pos, u64 &out_sum, uint32_t &out_klen) {
    const uint32_t lane = threadIdx.x;
    const u64 lanes_below = (1ull << lane) - 1ull;
    uint32_t first = 0;
    bool fresh = true;                                      // round 0 takes every position, a later one those marked 2
    for (;;) {
        for (uint32_t s = lane; s < AN_SET_SLOTS; s += 64u) {
            s_id[s] = -1;
            s_pos[s] = AN_EMPTY;
        }
        __syncthreads();
        uint32_t count = 0, next_first = len;
        for (uint32_t base = first; base < len; base += 64u) {
            const uint32_t p = base + lane;
            bool valid = p < len;
            if (valid && !fresh) valid = keep[b + p] == 2;
            const int32_t id = valid ? tok[b + p] : 0;
            // the fill mark is tested once per step: 64 more ids always fit, and an empty slot always remains
            const bool inserting = count <= AN_SET_FILL - 64u;
            bool found = false, is_new = false;
            uint32_t s = 0;
            if (valid) {
                const u64 h = fmix((u64)(uint32_t)id + 0x9E3779B97F4A7C15ull);
                s = (uint32_t)((flags & PGX_ANNOT_NARROW_HASH) ? (h & 7ull) : h) & (AN_SET_SLOTS - 1u);
                for (;;) {
                    const int32_t e = __hip_atomic_load(&s_id[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (e == id) { found = true; break; }
                    if (e == -1) {
                        if (!inserting) break;
                        const int32_t old = atomicCAS(&s_id[s], -1, id);
                        if (old == -1) { found = true; is_new = true; break; }
                        if (old == id) { found = true; break; }
                    }
                    s = (s + 1u) & (AN_SET_SLOTS - 1u);
                }
                if (found) atomicMin(&s_pos[s], p);
            }
            __syncthreads();
            count += (uint32_t)__popcll(__ballot(is_new));
            // positions are taken in ascending order, so the minimum of an id is final after the step that inserted it
            if (valid) {
                if (found)
                    keep[b + p] = __hip_atomic_load(&s_pos[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == p ? 1 : 0;
                else
                    keep[b + p] = 2;
            }
            const u64 pending = __ballot(valid && !found);
            if (pending && next_first == len) next_first = base + (uint32_t)__builtin_ctzll(pending);
            __syncthreads();
        }
        if (next_first == len) break;
        first = next_first;                                 // (> the first of this round: that position was inserted)
        fresh = false;
    }
    // every position is 0 or 1 now: places, the list and its hash
    uint32_t klen = 0;
    u64 sum = 0;
    for (uint32_t base = 0; base < len; base += 64u) {
        const uint32_t p = base + lane;
        const bool kept = p < len && keep[b + p] == 1;
        const u64 bits = __ballot(kept);
        if (kept) {
            const int32_t id = tok[b + p];
            const uint32_t place = klen + (uint32_t)__popcll(bits & lanes_below);
            ktok[b + place] = id;
            sum += id_mix(id, place);
        }
        klen += (uint32_t)__popcll(bits);
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = __shfl_xor((int)(uint32_t)sum, d, 64);
        const uint32_t hi = __shfl_xor((int)(uint32_t)(sum >> 32), d, 64);
        sum += ((u64)hi << 32) | lo;
    }
    out_sum = sum;
    out_klen = klen;
}

__global__ __launch_bounds__(64) void annot_long_rows_kernel(const int32_t *__restrict__ tok, const u64 *__restrict__ row_off,
                                                             uint32_t n_rows, u64 n_tokens, uint32_t flags, uint8_t *keep,
                                                             int32_t *__restrict__ ktok, u64 *__restrict__ row_hash,
                                                             uint32_t *__restrict__ row_klen) {
    __shared__ int32_t s_id[AN_SET_SLOTS];
    __shared__ uint32_t s_pos[AN_SET_SLOTS];
    const uint32_t lane = threadIdx.x;
    const uint32_t n_chunks = (n_rows + 63u) / 64u;
    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const uint32_t r = chunk * 64u + lane;
        u64 b = 0;
        uint32_t len = 0;
        if (r < n_rows) row_span(row_off, r, n_tokens, b, len);
        u64 todo = __ballot(r < n_rows && len > AN_ROW_TILE);       // the same on every lane: the wave takes them in turn
        while (todo) {
            const uint32_t j = (uint32_t)__builtin_ctzll(todo);
            todo &= todo - 1ull;
            const uint32_t rr = chunk * 64u + j;
            u64 rb;
            uint32_t rlen;
            row_span(row_off, rr, n_tokens, rb, rlen);
            u64 sum;
            uint32_t klen;
            long_row(tok, rb, rlen, flags, keep, ktok, s_id, s_pos, sum, klen);
            if (lane == 0u) {
                row_hash[rr] = list_hash(sum, klen, flags);
                row_klen[rr] = klen;
            }
        }
    }
}

// ---- runs -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AN_THREADS) void annot_short_runs_kernel(const int32_t *__restrict__ ktok,
                                                                      const u64 *__restrict__ row_off, uint32_t n_rows,
                                                                      u64 n_tokens, const uint32_t *__restrict__ run_off,
                                                                      uint32_t n_runs, const u64 *__restrict__ row_hash,
                                                                      const uint32_t *__restrict__ row_klen,
                                                                      int32_t *__restrict__ winner,
                                                                      uint32_t *__restrict__ votes,
                                                                      uint8_t *__restrict__ differs) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_waves = gridDim.x * AN_WAVES;
    // no barrier in here: a wave's trips are its own, and everything between lanes is a shuffle of the whole wave
    for (uint32_t u = blockIdx.x * AN_WAVES + (threadIdx.x >> 6); u < n_runs; u += n_waves) {
        uint32_t start, size;
        run_span(run_off, u, n_rows, start, size);
        if (size == 0u || size > AN_RUN_TILE) continue;
        const bool live = lane < size;
        const uint32_t r = start + lane;
        u64 h = 0, b = 0;
        uint32_t klen = 0;
        if (live) {
            uint32_t len;
            row_span(row_off, r, n_tokens, b, len);
            h = row_hash[r];
            klen = row_klen[r];
            klen = klen < len ? klen : len;
        }
        uint32_t rep = AN_NO_REP;
        for (uint32_t j = 0; j < size; ++j) {
            if ((uint32_t)__shfl((int)rep, (int)j, 64) != AN_NO_REP) continue;   // row j joined an earlier row: so did its equals
            const u64 hj = shfl_u64(h, (int)j), bj = shfl_u64(b, (int)j);
            const uint32_t kj = (uint32_t)__shfl((int)klen, (int)j, 64);
            if (live && rep == AN_NO_REP && lane >= j)
                if (lane == j || (h == hj && klen == kj && lists_equal(ktok, b, bj, klen))) rep = j;
        }
        uint32_t count = 0;
        for (uint32_t j = 0; j < size; ++j) count += (uint32_t)__shfl((int)rep, (int)j, 64) == rep ? 1u : 0u;
        uint32_t key = live ? (count << 8) | (63u - lane) : 0u;                   // (count <= 64)
        for (int d = 32; d >= 1; d >>= 1) {
            const uint32_t other = (uint32_t)__shfl_xor((int)key, d, 64);
            key = other > key ? other : key;
        }
        const uint32_t wlane = 63u - (key & 0xFFu);
        const uint32_t wrep = (uint32_t)__shfl((int)rep, (int)wlane, 64);
        if (live) differs[r] = rep != wrep ? 1 : 0;
        if (lane == 0u) {
            winner[u] = (int32_t)(start + wlane);
            votes[u] = key >> 8;
        }
    }
}

__global__ __launch_bounds__(AN_THREADS) void annot_long_runs_kernel(const int32_t *__restrict__ ktok,
                                                                     const u64 *__restrict__ row_off, uint32_t n_rows,
                                                                     u64 n_tokens, const uint32_t *__restrict__ run_off,
                                                                     uint32_t n_runs, const u64 *__restrict__ row_hash,
                                                                     const uint32_t *__restrict__ row_klen, uint32_t *t_rep,
                                                                     uint32_t *t_min, uint32_t *t_cnt, uint32_t *row_slot,
                                                                     int32_t *__restrict__ winner,
                                                                     uint32_t *__restrict__ votes,
                                                                     uint8_t *__restrict__ differs) {
    __shared__ u64 s_key[AN_WAVES];
    const uint32_t tid = threadIdx.x;
    for (uint32_t u = blockIdx.x; u < n_runs; u += gridDim.x) {    // (the same trips on every thread: barriers inside)
        uint32_t start, size;
        run_span(run_off, u, n_rows, start, size);
        if (size <= AN_RUN_TILE) continue;
        for (uint32_t i = tid; i < size; i += AN_THREADS) {
            const uint32_t r = start + i;
            u64 b;
            uint32_t len;
            row_span(row_off, r, n_tokens, b, len);
            const u64 h = row_hash[r];
            uint32_t klen = row_klen[r];
            klen = klen < len ? klen : len;
            uint32_t s = (uint32_t)(h % size);
            // the classes are at most `size` and a slot is never emptied: a row meets its class or an empty slot within
            // `size` probes (the bound only matters for a device caller whose runs overlap)
            for (uint32_t probes = 0; probes < size; ++probes) {
                uint32_t e = __hip_atomic_load(&t_rep[start + s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (e == AN_EMPTY) {
                    const uint32_t old = atomicCAS(&t_rep[start + s], AN_EMPTY, r);
                    e = old == AN_EMPTY ? r : old;
                }
                if (e == r) break;
                if (e < n_rows && row_hash[e] == h) {
                    u64 eb;
                    uint32_t elen;
                    row_span(row_off, e, n_tokens, eb, elen);
                    uint32_t eklen = row_klen[e];
                    eklen = eklen < elen ? eklen : elen;
                    if (eklen == klen && lists_equal(ktok, b, eb, klen)) break;
                }
                s = s + 1u == size ? 0u : s + 1u;
            }
            atomicMin(&t_min[start + s], r);                       // a minimum and a sum: any order
            atomicAdd(&t_cnt[start + s], 1u);
            row_slot[r] = s;
        }
        __threadfence();
        __syncthreads();
        u64 key = 0;
        for (uint32_t i = tid; i < size; i += AN_THREADS) {
            const uint32_t c = __hip_atomic_load(&t_cnt[start + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (c) {
                const uint32_t m = __hip_atomic_load(&t_min[start + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const u64 k = ((u64)c << 32) | (u64)(0xFFFFFFFFu - m);
                key = k > key ? k : key;
            }
        }
        for (int d = 32; d >= 1; d >>= 1) {
            const u64 other = shfl_u64(key, (int)((tid & 63u) ^ (uint32_t)d));
            key = other > key ? other : key;
        }
        if ((tid & 63u) == 0u) s_key[tid >> 6] = key;
        __syncthreads();
        key = s_key[0];
        for (uint32_t w = 1; w < AN_WAVES; ++w) key = s_key[w] > key ? s_key[w] : key;
        const uint32_t wrow = 0xFFFFFFFFu - (uint32_t)key;
        for (uint32_t i = tid; i < size; i += AN_THREADS) {
            const uint32_t r = start + i;
            uint32_t s = row_slot[r];                              // (this thread's own store)
            s = s < size ? s : 0u;
            const uint32_t m = __hip_atomic_load(&t_min[start + s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            differs[r] = m != wrow ? 1 : 0;
        }
        if (tid == 0u) {
            winner[u] = (int32_t)wrow;
            votes[u] = (uint32_t)(key >> 32);
        }
        __syncthreads();                                           // s_key is the next run's
    }
}

// ---- launches -------------------------------------------------------------------------------------------------------------
struct VoteWs {
    size_t ktok, row_hash, row_klen, t_rep_min, t_cnt, row_slot, bytes;
};

VoteWs vote_layout(uint32_t n_rows, u64 n_tokens) {
    VoteWs w;
    WsLayout lay;
    w.ktok = lay.take((size_t)n_tokens * 4);
    w.row_hash = lay.take((size_t)n_rows * 8);
    w.row_klen = lay.take((size_t)n_rows * 4);
    w.t_rep_min = lay.take((size_t)n_rows * 8);             // rep, then min: one fill with 0xFF
    w.t_cnt = lay.take((size_t)n_rows * 4);
    w.row_slot = lay.take((size_t)n_rows * 4);
    w.bytes = lay.off;
    return w;
}

int vote_sizes(pgx_ctx *ctx, uint32_t n_rows, u64 n_tokens, uint32_t n_runs, uint32_t flags) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(n_rows < AN_MAX_ROWS, "n_rows must be below 2^24");
    PGX_REQUIRE(n_tokens < AN_MAX_TOKENS, "n_tokens must be below 2^31");
    PGX_REQUIRE((flags & ~PGX_ANNOT_NARROW_HASH) == 0, "unknown flags");
    PGX_REQUIRE(n_runs <= n_rows && (n_runs > 0 || n_rows == 0), "runs are not empty and cover every row");
    return PGX_OK;
}

uint32_t capped(uint32_t blocks, uint32_t cap) { return blocks < cap ? (blocks ? blocks : 1u) : cap; }

// Only enqueues. n_rows >= 1.
int vote_launch(pgx_ctx *ctx, const int32_t *d_tok, const u64 *d_row_off, uint32_t n_rows, u64 n_tokens,
                const uint32_t *d_run_off, uint32_t n_runs, uint32_t flags, uint8_t *d_keep, int32_t *d_winner,
                uint32_t *d_votes, uint8_t *d_differs, uint8_t *ws, hipStream_t stream) {
    const VoteWs w = vote_layout(n_rows, n_tokens);
    int32_t *ktok = (int32_t *)(ws + w.ktok);
    u64 *row_hash = (u64 *)(ws + w.row_hash);
    uint32_t *row_klen = (uint32_t *)(ws + w.row_klen), *t_rep = (uint32_t *)(ws + w.t_rep_min), *t_min = t_rep + n_rows;
    uint32_t *t_cnt = (uint32_t *)(ws + w.t_cnt), *row_slot = (uint32_t *)(ws + w.row_slot);
    PGX_HIP(hipMemsetAsync(t_rep, 0xFF, (size_t)n_rows * 8, stream));
    PGX_HIP(hipMemsetAsync(t_cnt, 0, (size_t)n_rows * 4, stream));
    {
        ProfScope prof(ctx, "annot_rows_kernel", stream);
        annot_rows_kernel<<<capped(ceil_div_u32(n_rows, AN_GROUPS_PER_BLOCK), AN_MAX_GRID), AN_THREADS, 0, stream>>>(
            d_tok, d_row_off, n_rows, n_tokens, flags, d_keep, ktok, row_hash, row_klen);
    }
    {
        ProfScope prof(ctx, "annot_long_rows_kernel", stream);
        annot_long_rows_kernel<<<capped(ceil_div_u32(n_rows, 64u), AN_MAX_GRID), 64, 0, stream>>>(
            d_tok, d_row_off, n_rows, n_tokens, flags, d_keep, ktok, row_hash, row_klen);
    }
    PGX_HIP(hipGetLastError());
    {
        ProfScope prof(ctx, "annot_short_runs_kernel", stream);
        annot_short_runs_kernel<<<capped(ceil_div_u32(n_runs, AN_WAVES), AN_MAX_GRID), AN_THREADS, 0, stream>>>(
            ktok, d_row_off, n_rows, n_tokens, d_run_off, n_runs, row_hash, row_klen, d_winner, d_votes, d_differs);
    }
    {
        ProfScope prof(ctx, "annot_long_runs_kernel", stream);
        annot_long_runs_kernel<<<capped(n_runs, 2048u), AN_THREADS, 0, stream>>>(
            ktok, d_row_off, n_rows, n_tokens, d_run_off, n_runs, row_hash, row_klen, t_rep, t_min, t_cnt, row_slot,
            d_winner, d_votes, d_differs);
    }
    PGX_HIP(hipGetLastError());
    return PGX_OK;
}

int vote_dev(pgx_ctx *ctx, const int32_t *d_tok, const u64 *d_row_off, uint32_t n_rows, u64 n_tokens,
             const uint32_t *d_run_off, uint32_t n_runs, uint32_t flags, uint8_t *d_keep, int32_t *d_winner, uint32_t *d_votes,
             uint8_t *d_differs, void *d_ws, size_t ws_bytes, hipStream_t stream) {
    int rc = vote_sizes(ctx, n_rows, n_tokens, n_runs, flags);
    if (rc != PGX_OK) return rc;
    if (n_rows == 0) return PGX_OK;
    PGX_REQUIRE(d_row_off && d_run_off && d_winner && d_votes && d_differs, "NULL argument");
    PGX_REQUIRE(n_tokens == 0 || (d_tok && d_keep), "NULL tok or keep");
    PGX_REQUIRE(d_ws && ws_bytes >= vote_layout(n_rows, n_tokens).bytes,
                "workspace too small (see pgx_annot_vote_workspace_bytes)");
    PGX_REQUIRE(((uintptr_t)d_ws & 15u) == 0, "workspace must be 16-byte aligned");
    PGX_REQUIRE(((uintptr_t)d_row_off & 7u) == 0, "row_off must be 8-byte aligned");
    PGX_REQUIRE((((uintptr_t)d_tok | (uintptr_t)d_run_off | (uintptr_t)d_winner | (uintptr_t)d_votes) & 3u) == 0,
                "tok, run_off, winner and votes must be 4-byte aligned");
    rc = vote_launch(ctx, d_tok, d_row_off, n_rows, n_tokens, d_run_off, n_runs, flags, d_keep, d_winner, d_votes, d_differs,
                     (uint8_t *)d_ws, stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(hipStreamSynchronize(stream));
    return PGX_OK;
}

int vote_host(pgx_ctx *ctx, const int32_t *tok, const uint64_t *row_off, uint32_t n_rows, const uint32_t *run_off,
              uint32_t n_runs, uint32_t flags, uint8_t *out_keep, int32_t *out_winner, uint32_t *out_votes,
              uint8_t *out_differs) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(n_rows < AN_MAX_ROWS, "n_rows must be below 2^24");
    PGX_REQUIRE(row_off && run_off, "NULL row_off or run_off");
    PGX_REQUIRE(row_off[0] == 0, "row_off must start at 0");
    for (uint32_t r = 0; r < n_rows; ++r) PGX_REQUIRE(row_off[r] <= row_off[r + 1], "offsets must not decrease");
    const u64 n_tokens = row_off[n_rows];
    int rc = vote_sizes(ctx, n_rows, n_tokens, n_runs, flags);
    if (rc != PGX_OK) return rc;
    PGX_REQUIRE(run_off[0] == 0 && run_off[n_runs] == n_rows, "the runs must cover the rows");
    for (uint32_t u = 0; u < n_runs; ++u) PGX_REQUIRE(run_off[u] < run_off[u + 1], "a run is empty or out of range");
    PGX_REQUIRE(n_tokens == 0 || tok, "NULL tok");
    for (u64 p = 0; p < n_tokens; ++p) PGX_REQUIRE(tok[p] >= 0, "an id must not be negative");
    if (n_rows == 0) return PGX_OK;
    PGX_REQUIRE(out_winner && out_votes && out_differs && (n_tokens == 0 || out_keep), "NULL argument");
    PGX_HIP(hipSetDevice(ctx->device_id));
    DevBuf d_tok(ctx, AN_SLOT_TOK), d_ws(ctx, AN_SLOT_WS);
    DevPack in(ctx, AN_SLOT_OFFSETS), res(ctx, AN_SLOT_RESULT);
    const PackPart rows = in.in(row_off, (size_t)n_rows + 1), runs = in.in(run_off, (size_t)n_runs + 1);
    const PackPart keep = res.out(out_keep, (size_t)n_tokens), winner = res.out(out_winner, n_runs),
                   votes = res.out(out_votes, n_runs), differs = res.out(out_differs, n_rows);
    PGX_HIP(d_tok.alloc((size_t)n_tokens * 4));
    PGX_HIP(in.alloc());
    PGX_HIP(res.alloc());
    PGX_HIP(d_ws.alloc(vote_layout(n_rows, n_tokens).bytes));
    if (n_tokens) {
        rc = pgx_staged_h2d(ctx, d_tok.p, tok, (size_t)n_tokens * 4, ctx->stream);
        if (rc != PGX_OK) return rc;
    }
    PGX_HIP(in.upload(ctx->stream));
    rc = vote_launch(ctx, d_tok.as<int32_t>(), in.dev<u64>(rows), n_rows, n_tokens, in.dev<uint32_t>(runs), n_runs, flags,
                     res.dev<uint8_t>(keep), res.dev<int32_t>(winner), res.dev<uint32_t>(votes), res.dev<uint8_t>(differs),
                     d_ws.as<uint8_t>(), ctx->stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(res.download(ctx->stream));
    PGX_HIP(hipStreamSynchronize(ctx->stream));
    return PGX_OK;
}

}  // namespace

extern "C" {

uint32_t pgx_annot_row_tile(void) { return AN_ROW_TILE; }

uint32_t pgx_annot_run_tile(void) { return AN_RUN_TILE; }

size_t pgx_annot_vote_workspace_bytes(uint32_t n_rows, uint64_t n_tokens, uint32_t n_runs) {
    if (n_rows >= AN_MAX_ROWS || n_tokens >= AN_MAX_TOKENS || n_runs > n_rows) return 0;
    return vote_layout(n_rows, n_tokens).bytes;
}

int pgx_annot_vote(pgx_ctx *ctx, const int32_t *tok, const uint64_t *row_off, uint32_t n_rows, const uint32_t *run_off,
                   uint32_t n_runs, uint32_t flags, uint8_t *out_keep, int32_t *out_winner, uint32_t *out_votes,
                   uint8_t *out_differs) {
    return guarded(__func__, [&] {
        return vote_host(ctx, tok, row_off, n_rows, run_off, n_runs, flags, out_keep, out_winner, out_votes, out_differs);
    });
}

int pgx_annot_vote_dev(pgx_ctx *ctx, const int32_t *d_tok, const uint64_t *d_row_off, uint32_t n_rows, uint64_t n_tokens,
                       const uint32_t *d_run_off, uint32_t n_runs, uint32_t flags, uint8_t *d_keep, int32_t *d_winner,
                       uint32_t *d_votes, uint8_t *d_differs, void *d_workspace, size_t workspace_bytes, void *stream) {
    return guarded(__func__, [&] {
        return vote_dev(ctx, d_tok, (const u64 *)d_row_off, n_rows, n_tokens, d_run_off, n_runs, flags, d_keep, d_winner,
                        d_votes, d_differs, d_workspace, workspace_bytes, (hipStream_t)stream);
    });
}

}  // extern "C"
