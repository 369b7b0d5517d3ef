// The two device steps of the proximal (5'/3' UTR) pangenome builders (reference pangenome.py:900-1184, which slices one
// window per GFF line out of a Python string and keeps one dictionary of sequences per gene):
//   cut     windows of a text gathered end to end into one blob; a reverse window comes out reverse-complemented
//   group   records (a byte string each, keyed by a gene id) grouped exactly: first[i] = the smallest record equal to record
//           i in gene, length and bytes; variant[i] = how many distinct records of i's gene appear before first[i]
// Both are functions of the input alone: no atomic decides an order or a value (the only atomics are the CAS that claims a
// hash slot, whose result is read through a minimum over a set, and LDS counters that are only ever summed).
//
// cut: a group of PX_GROUP lanes owns one window and walks the ALIGNED 16-byte words of its piece of the output, a lane a
// word. A word that lies inside the piece is one 16-byte store; the two ragged ends are stored byte by byte, because the
// other bytes of those words belong to the neighbouring windows. The source bytes come through load_chunk (aligned 16-byte
// loads inside the text, single bytes at its edges); a reverse window reads the mirrored span and maps it through a
// 256-entry table in LDS, back to front. A byte outside the table becomes 0 and raises bad[i].
//
// group: dict.hip's open-addressed table (string_hash.h) with the gene mixed into hash and tag and compared before the
// length. Then the variant numbers: the records are sorted stably by gene (three passes of a counting sort on 8-bit digits:
// a wave owns a tile of PX_TILE records, counts it, and after one scan of the digit-major count matrix places it in index
// order, the lanes of a step ranked by ballots), the "is its own first" flags are scanned in that order, and a record's
// number is its prefix minus the prefix at its gene's first sorted position (a binary search). O(N) memory, O(N log N)
// work however the records spread over the genes.
#include "pgx_internal.h"
#include "string_hash.h"

namespace {

using namespace string_hash;

constexpr int PX_THREADS = 256;
constexpr uint32_t PX_GROUP = DM_GROUP;                    // lanes per window / record
constexpr uint32_t PX_STEP = PX_GROUP * DM_CHUNK;          // output bytes per group and step (pgx_prox_cut_group_bytes)
constexpr uint32_t PX_GROUPS_PER_BLOCK = PX_THREADS / PX_GROUP;
constexpr uint32_t PX_MAX_GRID = 8192;
constexpr u64 PX_EMPTY = ~0ull;
constexpr uint32_t PX_MAX_N = 1u << 24;                    // records / windows: an index fits an entry's low 24 bits
constexpr uint32_t PX_MAX_GENE = 1u << 24;
constexpr uint32_t PX_DIGIT_BITS = 8, PX_BINS = 1u << PX_DIGIT_BITS, PX_PASSES = 3;   // 3 x 8 bits = a gene id
constexpr uint32_t PX_WAVES = PX_THREADS / 64;
constexpr uint32_t PX_TILE = 1024;                         // records per wave and sort pass (pgx_prox_group_tile)
constexpr uint32_t PX_TILE_STEPS = PX_TILE / 64;
constexpr uint32_t PX_SCAN_PER_THREAD = 8, PX_SCAN_TILE = PX_THREADS * PX_SCAN_PER_THREAD;
static_assert(PX_DIGIT_BITS * PX_PASSES == 24, "the passes cover a gene id");

// comp[b] of the reference's reverse_complement; 0 = no such base
__device__ __forceinline__ uint32_t complement_of(uint32_t b) {
    const char *from = "ACGTWSRYMKNacgtwsrymkn", *to = "TGCAWSYRKMNtgcawsyrkmn";
    uint32_t r = 0;
    for (int j = 0; j < 22; ++j) r = b == (uint32_t)(uint8_t)from[j] ? (uint32_t)(uint8_t)to[j] : r;
    return r;
}

// The 16 bytes of c reversed and complemented (byte j of the result = comp of byte 15 - j); `bad` is raised by a byte among the
// first n of the RESULT (the last n of c) that has no complement.
__device__ __forceinline__ Chunk reverse_complement_chunk(const Chunk &c, const uint8_t *s_comp, uint32_t n, bool &bad) {
    Chunk r;
    r.lo = r.hi = 0;
    for (uint32_t j = 0; j < 16u; ++j) {
        const uint32_t src = 15u - j;
        const uint32_t b = (uint32_t)((src < 8u ? c.lo >> (src * 8u) : c.hi >> ((src - 8u) * 8u)) & 0xFFull);
        const u64 m = s_comp[b];
        bad |= j < n && m == 0ull;
        if (j < 8u) r.lo |= m << (j * 8u);
        else r.hi |= m << ((j - 8u) * 8u);
    }
    return r;
}

__global__ __launch_bounds__(PX_THREADS) void prox_cut_kernel(const uint8_t *__restrict__ text, u64 text_bytes,
                                                              const u64 *__restrict__ start,
                                                              const uint32_t *__restrict__ length,
                                                              const uint8_t *__restrict__ reverse,
                                                              const u64 *__restrict__ out_offsets, uint32_t n,
                                                              uint8_t *__restrict__ out, uint8_t *__restrict__ bad) {
    __shared__ uint8_t s_comp[256];
    s_comp[threadIdx.x] = (uint8_t)complement_of(threadIdx.x);
    __syncthreads();
    const uint32_t sub = threadIdx.x & (PX_GROUP - 1u);
    const uint32_t lane = threadIdx.x & 63u;
    const u64 group_lanes = ((1ull << PX_GROUP) - 1ull) << (lane & ~(PX_GROUP - 1u));
    const uint32_t n_rounds = (n + PX_GROUPS_PER_BLOCK - 1u) / PX_GROUPS_PER_BLOCK;
    // every lane takes the same number of rounds, so the ballot is reached by whole waves
    for (uint32_t round = blockIdx.x; round < n_rounds; round += gridDim.x) {
        const uint32_t i = round * PX_GROUPS_PER_BLOCK + threadIdx.x / PX_GROUP;
        const bool live = i < n;
        u64 s = 0, len = 0;
        bool rev = false, is_bad = false;
        uint8_t *dst = out;
        if (live) {
            // clamped into the text whatever the arrays hold (the host entry has checked them)
            s = start[i];
            s = s < text_bytes ? s : text_bytes;
            len = length[i];
            len = len < text_bytes - s ? len : text_bytes - s;
            rev = reverse[i] != 0;
            dst = out + out_offsets[i];
        }
        // the piece is dst[0 .. len); word w of it is the aligned 16 bytes at dst - mis + 16 w
        const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u);
        const u64 n_words = len ? (mis + len + 15u) / 16u : 0;
        for (u64 w = sub; w < n_words; w += PX_GROUP) {
            // bytes [k0, k1) of the window go to this word
            const u64 k0 = w == 0 ? 0 : w * 16u - mis;
            const u64 k1 = (w + 1u) * 16u - mis < len ? (w + 1u) * 16u - mis : len;
            const uint32_t cnt = (uint32_t)(k1 - k0);
            Chunk c;
            if (!rev) c = load_chunk(text, text_bytes, s + k0, cnt);
            else {
                // out[k] = comp(text[s + len - 1 - k]): the cnt bytes that end at s + len - k0, loaded so that they are the
                // LAST cnt of a 16-byte chunk, which the mirror turns into the first cnt
                const Chunk raw = load_chunk(text, text_bytes, s + len - k1, cnt);
                Chunk hi_aligned;
                const uint32_t sh = (16u - cnt) * 8u;      // move the cnt low bytes to the top
                if (sh == 0u) hi_aligned = raw;
                else if (sh >= 64u) { hi_aligned.lo = 0; hi_aligned.hi = sh == 64u ? raw.lo : raw.lo << (sh - 64u); }
                else { hi_aligned.hi = (raw.hi << sh) | (raw.lo >> (64u - sh)); hi_aligned.lo = raw.lo << sh; }
                c = reverse_complement_chunk(hi_aligned, s_comp, cnt, is_bad);
            }
            uint8_t *p = dst + k0;
            if (cnt == 16u) *reinterpret_cast<uint4 *>(p) = make_uint4((uint32_t)c.lo, (uint32_t)(c.lo >> 32), (uint32_t)c.hi,
                                                                        (uint32_t)(c.hi >> 32));
            else
                for (uint32_t j = 0; j < cnt; ++j) p[j] = (uint8_t)(j < 8u ? c.lo >> (j * 8u) : c.hi >> ((j - 8u) * 8u));
        }
        const u64 votes = __ballot(is_bad) & group_lanes;
        if (live && sub == 0u) bad[i] = votes != 0ull ? 1 : 0;
    }
}

// ---- group: first -----------------------------------------------------------------------------------------------------------
uint32_t prox_slots(uint32_t n) {
    uint32_t slots = 64;
    while (slots < 2 * n) slots <<= 1;                     // (n < 2^24: at most 2^25)
    return slots;
}

__device__ __forceinline__ u64 record_hash(const uint8_t *__restrict__ blob, u64 total, u64 begin, u64 len, uint32_t gene,
                                           uint32_t sub, uint32_t flags, Chunk &first) {
    const u64 h = fmix(group_hash(blob, total, begin, len, sub, 0u, first) ^ ((u64)gene + 1ull) * 0x9E3779B97F4A7C15ull);
    return (flags & PGX_PROX_NARROW_HASH) ? (h & 7ull) : h;
}

__global__ __launch_bounds__(PX_THREADS) void prox_build_kernel(const uint8_t *__restrict__ blob,
                                                                const u64 *__restrict__ offsets,
                                                                const int32_t *__restrict__ gene, uint32_t n, uint32_t flags,
                                                                u64 *table, uint32_t mask) {
    const uint32_t sub = threadIdx.x & (PX_GROUP - 1u);
    const u64 total = offsets[n];
    const uint32_t n_rounds = (n + PX_GROUPS_PER_BLOCK - 1u) / PX_GROUPS_PER_BLOCK;
    for (uint32_t round = blockIdx.x; round < n_rounds; round += gridDim.x) {
        const uint32_t k = round * PX_GROUPS_PER_BLOCK + threadIdx.x / PX_GROUP;
        const bool live = k < n;
        u64 begin = 0, len = 0;
        if (live) string_span(offsets, k, total, begin, len);
        Chunk first;
        const u64 h = record_hash(blob, total, begin, len, live ? (uint32_t)gene[k] : 0u, sub, flags, first);
        if (!live || sub != 0u) continue;
        const u64 entry = ((h >> 24) << 24) | k;
        uint32_t s = (uint32_t)h & mask;
        // `mask + 1` >= 2 n slots, of which fewer than n are taken: an empty one is always met
        for (;;) {
            if (__atomic_load_n(&table[s], __ATOMIC_RELAXED) == PX_EMPTY && atomicCAS(&table[s], PX_EMPTY, entry) == PX_EMPTY)
                break;
            s = (s + 1u) & mask;
        }
    }
}

// first[i] = the smallest index among the records equal to record i (itself included): a minimum over a set, whatever
// order the records were inserted in.
__global__ __launch_bounds__(PX_THREADS) void prox_first_kernel(const uint8_t *__restrict__ blob,
                                                                const u64 *__restrict__ offsets,
                                                                const int32_t *__restrict__ gene, uint32_t n, uint32_t flags,
                                                                const u64 *__restrict__ table, uint32_t mask,
                                                                int32_t *__restrict__ first_out) {
    const uint32_t sub = threadIdx.x & (PX_GROUP - 1u);
    const uint32_t lane = threadIdx.x & 63u;
    const u64 group_lanes = ((1ull << PX_GROUP) - 1ull) << (lane & ~(PX_GROUP - 1u));
    const u64 total = offsets[n];
    const uint32_t n_rounds = (n + PX_GROUPS_PER_BLOCK - 1u) / PX_GROUPS_PER_BLOCK;
    for (uint32_t round = blockIdx.x; round < n_rounds; round += gridDim.x) {
        const uint32_t i = round * PX_GROUPS_PER_BLOCK + threadIdx.x / PX_GROUP;
        const bool live = i < n;
        u64 begin = 0, len = 0;
        if (live) string_span(offsets, i, total, begin, len);
        const int32_t g = live ? gene[i] : 0;
        Chunk first;
        const u64 h = record_hash(blob, total, begin, len, (uint32_t)g, sub, flags, first);
        const u64 tag = h >> 24;
        const u64 n_chunks = (len + DM_CHUNK - 1) / DM_CHUNK;
        uint32_t best = i;
        // live, s, e, k and the candidate's span are the same on every lane of a group, so a group leaves the walk as one;
        // the vote is taken by every lane still walking, a lane that has nothing to compare voting "equal"
        bool walking = live;
        uint32_t s = (uint32_t)h & mask;
        while (walking) {
            const u64 e = table[s];
            s = (s + 1u) & mask;
            bool differs = false, candidate = false;
            uint32_t k = 0;
            if (e == PX_EMPTY) walking = false;
            else if ((e >> 24) == tag) {
                k = (uint32_t)e & 0xFFFFFFu;
                k = k < n ? k : i;
                u64 kb, kl;
                string_span(offsets, k, total, kb, kl);
                candidate = k < best && gene[k] == g && kl == len;
                if (candidate) {
                    for (u64 c = sub; c < n_chunks; c += PX_GROUP) {
                        const u64 left = len - c * DM_CHUNK;
                        const uint32_t m = left < DM_CHUNK ? (uint32_t)left : DM_CHUNK;
                        const Chunk q = c == sub ? first : load_chunk(blob, total, begin + c * DM_CHUNK, m);
                        const Chunk t = load_chunk(blob, total, kb + c * DM_CHUNK, m);
                        differs |= (q.lo != t.lo) | (q.hi != t.hi);
                    }
                }
            }
            const u64 votes = __ballot(differs) & group_lanes;
            if (candidate && votes == 0ull) best = k;
        }
        if (live && sub == 0u) first_out[i] = (int32_t)best;
    }
}

// ---- exclusive scan of uint32 in place: sums of PX_SCAN_TILE elements, their scan by one workgroup, the tiles ----------------
// exclusive prefix of v over the workgroup's threads; *total = the sum, on every thread
__device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t *s_wave, uint32_t *total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)inc, d, 64);
        if (lane >= (uint32_t)d) inc += up;
    }
    __syncthreads();                                       // (s_wave may still be read from the call before)
    if (lane == 63u) s_wave[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < PX_WAVES; ++w) {
        before += w < wave ? s_wave[w] : 0u;
        all += s_wave[w];
    }
    *total = all;
    return before + inc - v;
}

__global__ __launch_bounds__(PX_THREADS) void prox_scan_sums_kernel(const uint32_t *__restrict__ a, uint32_t n,
                                                                    uint32_t *__restrict__ sums) {
    __shared__ uint32_t s_wave[PX_WAVES];
    const uint32_t base = blockIdx.x * PX_SCAN_TILE + threadIdx.x * PX_SCAN_PER_THREAD;
    uint32_t v = 0;
    for (uint32_t j = 0; j < PX_SCAN_PER_THREAD; ++j) v += base + j < n ? a[base + j] : 0u;
    uint32_t total;
    (void)block_exclusive(v, s_wave, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(PX_THREADS) void prox_scan_spine_kernel(uint32_t *sums, uint32_t n_sums) {
    __shared__ uint32_t s_wave[PX_WAVES];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_sums; base += PX_THREADS) {        // (the same trips on every thread)
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < n_sums ? sums[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive(v, s_wave, &total);
        if (i < n_sums) sums[i] = carry + ex;
        carry += total;
    }
}

__global__ __launch_bounds__(PX_THREADS) void prox_scan_apply_kernel(uint32_t *a, uint32_t n,
                                                                     const uint32_t *__restrict__ sums) {
    __shared__ uint32_t s_wave[PX_WAVES];
    const uint32_t base = blockIdx.x * PX_SCAN_TILE + threadIdx.x * PX_SCAN_PER_THREAD;
    uint32_t x[PX_SCAN_PER_THREAD], v = 0;
    for (uint32_t j = 0; j < PX_SCAN_PER_THREAD; ++j) {
        x[j] = base + j < n ? a[base + j] : 0u;
        v += x[j];
    }
    uint32_t total;
    uint32_t run = sums[blockIdx.x] + block_exclusive(v, s_wave, &total);
    for (uint32_t j = 0; j < PX_SCAN_PER_THREAD; ++j) {
        if (base + j < n) a[base + j] = run;
        run += x[j];
    }
}

// ---- group: stable counting sort of the record indices by one digit of the gene ----------------------------------------------
__device__ __forceinline__ uint32_t digit_of(const int32_t *__restrict__ gene, uint32_t idx, uint32_t shift) {
    return ((uint32_t)gene[idx] >> shift) & (PX_BINS - 1u);
}

// counts[d * n_tiles + t] = records of tile t whose digit is d. order_in NULL: the identity.
__global__ __launch_bounds__(PX_THREADS) void prox_sort_count_kernel(const int32_t *__restrict__ gene,
                                                                     const uint32_t *__restrict__ order_in, uint32_t n,
                                                                     uint32_t shift, uint32_t n_tiles,
                                                                     uint32_t *__restrict__ counts) {
    __shared__ uint32_t s_cnt[PX_WAVES][PX_BINS];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t tile = blockIdx.x * PX_WAVES + wave;
    for (uint32_t d = lane; d < PX_BINS; d += 64u) s_cnt[wave][d] = 0;
    __syncthreads();
    for (uint32_t step = 0; step < PX_TILE_STEPS; ++step) {
        const u64 p = (u64)tile * PX_TILE + step * 64u + lane;
        if (p < n) {
            const uint32_t idx = order_in ? order_in[p] : (uint32_t)p;
            atomicAdd(&s_cnt[wave][digit_of(gene, idx < n ? idx : 0u, shift)], 1u);     // (a sum: any order)
        }
    }
    __syncthreads();
    if (tile < n_tiles)
        for (uint32_t d = lane; d < PX_BINS; d += 64u) counts[(size_t)d * n_tiles + tile] = s_cnt[wave][d];
}

// bases = the exclusive scan of counts. A wave walks its tile in index order, 64 records a step; the records of a step that
// share a digit are ranked by lane (ballots), so equal digits keep their order: the sort is stable.
__global__ __launch_bounds__(PX_THREADS) void prox_sort_place_kernel(const int32_t *__restrict__ gene,
                                                                     const uint32_t *__restrict__ order_in, uint32_t n,
                                                                     uint32_t shift, uint32_t n_tiles,
                                                                     const uint32_t *__restrict__ bases,
                                                                     uint32_t *__restrict__ order_out) {
    __shared__ uint32_t s_pos[PX_WAVES][PX_BINS];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t tile = blockIdx.x * PX_WAVES + wave;
    for (uint32_t d = lane; d < PX_BINS; d += 64u) s_pos[wave][d] = tile < n_tiles ? bases[(size_t)d * n_tiles + tile] : 0u;
    __syncthreads();
    const u64 below = (1ull << lane) - 1ull;
    for (uint32_t step = 0; step < PX_TILE_STEPS; ++step) {             // (the same trips on every wave: barriers inside)
        const u64 p = (u64)tile * PX_TILE + step * 64u + lane;
        const bool valid = p < n;
        uint32_t idx = 0, d = 0;
        if (valid) {
            idx = order_in ? order_in[p] : (uint32_t)p;
            idx = idx < n ? idx : 0u;
            d = digit_of(gene, idx, shift);
        }
        u64 peers = __ballot(valid);
        for (uint32_t b = 0; b < PX_DIGIT_BITS; ++b) {
            const u64 set = __ballot((d >> b) & 1u);
            peers &= ((d >> b) & 1u) ? set : ~set;
        }
        const uint32_t before = (uint32_t)__popcll(peers & below);
        uint32_t pos = 0;
        if (valid) pos = s_pos[wave][d] + before;
        __syncthreads();
        if (valid && (peers >> lane) == 1ull) s_pos[wave][d] = pos + 1u;      // the last of its peers
        __syncthreads();
        if (valid && pos < n) order_out[pos] = idx;
    }
}

// In sorted order: the gene of every position, and 1 where the record is its own first.
__global__ __launch_bounds__(PX_THREADS) void prox_sorted_flags_kernel(const int32_t *__restrict__ gene,
                                                                       const int32_t *__restrict__ first,
                                                                       const uint32_t *__restrict__ order, uint32_t n,
                                                                       uint32_t *__restrict__ sorted_gene,
                                                                       uint32_t *__restrict__ flag) {
    const uint32_t p = blockIdx.x * PX_THREADS + threadIdx.x;
    if (p >= n) return;
    uint32_t i = order[p];
    i = i < n ? i : 0u;
    sorted_gene[p] = (uint32_t)gene[i] & (PX_MAX_GENE - 1u);
    flag[p] = first[i] == (int32_t)i ? 1u : 0u;
}

// prefix = the exclusive scan of the flags. A record that is its own first gets its number: the firsts before it in sorted
// order minus those before its gene's first position. The last position also gives the number of distinct records.
__global__ __launch_bounds__(PX_THREADS) void prox_rank_kernel(const int32_t *__restrict__ first,
                                                               const uint32_t *__restrict__ order, uint32_t n,
                                                               const uint32_t *__restrict__ sorted_gene,
                                                               const uint32_t *__restrict__ prefix,
                                                               int32_t *__restrict__ variant, uint32_t *__restrict__ n_distinct) {
    const uint32_t p = blockIdx.x * PX_THREADS + threadIdx.x;
    if (p >= n) return;
    uint32_t i = order[p];
    i = i < n ? i : 0u;
    const bool own = first[i] == (int32_t)i;
    if (p == n - 1u) *n_distinct = prefix[p] + (own ? 1u : 0u);
    if (!own) return;
    const uint32_t g = sorted_gene[p];
    uint32_t lo = 0, hi = p;                               // the smallest position whose gene is g
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (sorted_gene[mid] < g) lo = mid + 1u;
        else hi = mid;
    }
    variant[i] = (int32_t)(prefix[p] - prefix[lo]);
}

// every other record takes the number of its first (written by the kernel before, not by this one)
__global__ __launch_bounds__(PX_THREADS) void prox_variant_kernel(const int32_t *__restrict__ first, uint32_t n,
                                                                  int32_t *variant) {
    const uint32_t i = blockIdx.x * PX_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t f = (uint32_t)first[i];
    if (f != i) variant[i] = variant[f < n ? f : i];
}

// ---- launches -----------------------------------------------------------------------------------------------------------------
uint32_t rounds_grid(uint32_t n) {
    const uint32_t rounds = ceil_div_u32(n, PX_GROUPS_PER_BLOCK);
    return rounds < PX_MAX_GRID ? rounds : PX_MAX_GRID;
}

int cut_launch(pgx_ctx *ctx, const uint8_t *d_text, u64 text_bytes, const u64 *d_start, const uint32_t *d_length,
               const uint8_t *d_reverse, const u64 *d_out_offsets, uint32_t n, uint8_t *d_out, uint8_t *d_bad,
               hipStream_t stream) {
    if (n == 0) return PGX_OK;
    {
        ProfScope prof(ctx, "prox_cut_kernel", stream);
        prox_cut_kernel<<<rounds_grid(n), PX_THREADS, 0, stream>>>(d_text, text_bytes, d_start, d_length, d_reverse,
                                                                  d_out_offsets, n, d_out, d_bad);
    }
    PGX_HIP(hipGetLastError());
    return PGX_OK;
}

int cut_dev(pgx_ctx *ctx, const uint8_t *d_text, u64 text_bytes, const u64 *d_start, const uint32_t *d_length,
            const uint8_t *d_reverse, const u64 *d_out_offsets, uint32_t n, uint8_t *d_out, uint8_t *d_bad,
            hipStream_t stream) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(text_bytes < (1ull << 32), "text_bytes must be below 2^32");
    PGX_REQUIRE(n < PX_MAX_N, "n must be below 2^24");
    if (n == 0) return PGX_OK;
    PGX_REQUIRE(d_start && d_length && d_reverse && d_out_offsets && d_out && d_bad, "NULL argument");
    PGX_REQUIRE(text_bytes == 0 || d_text, "NULL text");
    PGX_REQUIRE(((uintptr_t)d_start & 7u) == 0 && ((uintptr_t)d_out_offsets & 7u) == 0 && ((uintptr_t)d_length & 3u) == 0,
                "start and out_offsets must be 8-byte aligned, length 4-byte aligned");
    int rc = cut_launch(ctx, d_text, text_bytes, d_start, d_length, d_reverse, d_out_offsets, n, d_out, d_bad, stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(hipStreamSynchronize(stream));
    return PGX_OK;
}

int cut_host(pgx_ctx *ctx, const uint8_t *text, u64 text_bytes, const uint64_t *start, const uint32_t *length,
             const uint8_t *reverse, uint32_t n, uint8_t *out, uint8_t *out_bad) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(text_bytes < (1ull << 32), "text_bytes must be below 2^32");
    PGX_REQUIRE(n < PX_MAX_N, "n must be below 2^24");
    if (n == 0) return PGX_OK;
    PGX_REQUIRE(start && length && reverse && out_bad, "NULL argument");
    PGX_REQUIRE(text_bytes == 0 || text, "NULL text");
    HostVec<uint64_t> off(ctx, PX_HOST_OFFSETS, (size_t)n + 1);
    PGX_REQUIRE(off.ok(), "out of host memory");
    u64 total = 0;
    for (uint32_t i = 0; i < n; ++i) {
        PGX_REQUIRE(start[i] <= text_bytes && length[i] <= text_bytes - start[i], "a window leaves the text");
        off[i] = total;
        total += length[i];
    }
    off[n] = total;
    PGX_REQUIRE(total < (1ull << 32), "the output must hold fewer than 2^32 bytes");
    PGX_REQUIRE(total == 0 || out, "NULL out");
    PGX_HIP(hipSetDevice(ctx->device_id));
    DevBuf d_text(ctx, PX_SLOT_TEXT);
    DevPack win(ctx, PX_SLOT_WINDOWS), res(ctx, PX_SLOT_OUT);
    const PackPart w_start = win.in(start, n), w_off = win.in(off.data(), (size_t)n + 1), w_len = win.in(length, n),
                   w_rev = win.in(reverse, n);
    const PackPart r_out = res.out(out, (size_t)total), r_bad = res.out(out_bad, n);
    PGX_HIP(d_text.alloc((size_t)text_bytes));
    PGX_HIP(win.alloc());
    PGX_HIP(res.alloc());
    if (text_bytes) {
        int rc = pgx_staged_h2d(ctx, d_text.p, text, (size_t)text_bytes, ctx->stream);
        if (rc != PGX_OK) return rc;
    }
    PGX_HIP(win.upload(ctx->stream));
    int rc = cut_launch(ctx, d_text.as<uint8_t>(), text_bytes, win.dev<u64>(w_start), win.dev<uint32_t>(w_len),
                        win.dev<uint8_t>(w_rev), win.dev<u64>(w_off), n, res.dev<uint8_t>(r_out), res.dev<uint8_t>(r_bad),
                        ctx->stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(res.download(ctx->stream));
    PGX_HIP(hipStreamSynchronize(ctx->stream));
    return PGX_OK;
}

struct GroupWs {
    size_t table, order_a, order_b, counts, sums, sorted_gene, prefix, bytes;
    uint32_t n_tiles, n_counts;
};

GroupWs group_layout(uint32_t n) {
    GroupWs g;
    WsLayout lay;
    g.n_tiles = ceil_div_u32(n, PX_TILE);
    g.n_counts = g.n_tiles * PX_BINS;                      // (n < 2^24: at most 2^22)
    const uint32_t longest = g.n_counts > n ? g.n_counts : n;
    g.table = lay.take((size_t)prox_slots(n) * 8);
    g.order_a = lay.take((size_t)n * 4);
    g.order_b = lay.take((size_t)n * 4);
    g.counts = lay.take((size_t)g.n_counts * 4);
    g.sums = lay.take((size_t)ceil_div_u32(longest, PX_SCAN_TILE) * 4);
    g.sorted_gene = lay.take((size_t)n * 4);
    g.prefix = lay.take((size_t)n * 4);
    g.bytes = lay.off;
    return g;
}

int scan_in_place(pgx_ctx *ctx, uint32_t *d_a, uint32_t n, uint32_t *d_sums, hipStream_t stream) {
    const uint32_t blocks = ceil_div_u32(n, PX_SCAN_TILE);
    ProfScope prof(ctx, "prox_scan_kernels", stream);
    prox_scan_sums_kernel<<<blocks, PX_THREADS, 0, stream>>>(d_a, n, d_sums);
    prox_scan_spine_kernel<<<1, PX_THREADS, 0, stream>>>(d_sums, blocks);
    prox_scan_apply_kernel<<<blocks, PX_THREADS, 0, stream>>>(d_a, n, d_sums);
    return PGX_OK;
}

int group_sizes(pgx_ctx *ctx, uint32_t n, uint32_t flags) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(n < PX_MAX_N, "n must be below 2^24");
    PGX_REQUIRE((flags & ~PGX_PROX_NARROW_HASH) == 0, "unknown flags");
    return PGX_OK;
}

// Only enqueues. n >= 1.
int group_launch(pgx_ctx *ctx, const uint8_t *d_blob, const u64 *d_offsets, const int32_t *d_gene, uint32_t n,
                 uint32_t flags, int32_t *d_first, int32_t *d_variant, uint32_t *d_distinct, uint8_t *ws,
                 hipStream_t stream) {
    const GroupWs g = group_layout(n);
    u64 *table = (u64 *)(ws + g.table);
    uint32_t *order[2] = {(uint32_t *)(ws + g.order_a), (uint32_t *)(ws + g.order_b)};
    uint32_t *counts = (uint32_t *)(ws + g.counts), *sums = (uint32_t *)(ws + g.sums);
    uint32_t *sorted_gene = (uint32_t *)(ws + g.sorted_gene), *prefix = (uint32_t *)(ws + g.prefix);
    const uint32_t slots = prox_slots(n);
    PGX_HIP(hipMemsetAsync(table, 0xFF, (size_t)slots * 8, stream));
    {
        ProfScope prof(ctx, "prox_build_kernel", stream);
        prox_build_kernel<<<rounds_grid(n), PX_THREADS, 0, stream>>>(d_blob, d_offsets, d_gene, n, flags, table, slots - 1u);
    }
    {
        ProfScope prof(ctx, "prox_first_kernel", stream);
        prox_first_kernel<<<rounds_grid(n), PX_THREADS, 0, stream>>>(d_blob, d_offsets, d_gene, n, flags, table, slots - 1u,
                                                                    d_first);
    }
    PGX_HIP(hipGetLastError());
    const uint32_t sort_blocks = ceil_div_u32(g.n_tiles, PX_WAVES), flat_blocks = ceil_div_u32(n, PX_THREADS);
    const uint32_t *in = nullptr;
    for (uint32_t pass = 0; pass < PX_PASSES; ++pass) {
        uint32_t *out = order[pass & 1u];
        {
            ProfScope prof(ctx, "prox_sort_count_kernel", stream);
            prox_sort_count_kernel<<<sort_blocks, PX_THREADS, 0, stream>>>(d_gene, in, n, pass * PX_DIGIT_BITS, g.n_tiles,
                                                                          counts);
        }
        int rc = scan_in_place(ctx, counts, g.n_counts, sums, stream);
        if (rc != PGX_OK) return rc;
        {
            ProfScope prof(ctx, "prox_sort_place_kernel", stream);
            prox_sort_place_kernel<<<sort_blocks, PX_THREADS, 0, stream>>>(d_gene, in, n, pass * PX_DIGIT_BITS, g.n_tiles,
                                                                          counts, out);
        }
        PGX_HIP(hipGetLastError());
        in = out;
    }
    {
        ProfScope prof(ctx, "prox_sorted_flags_kernel", stream);
        prox_sorted_flags_kernel<<<flat_blocks, PX_THREADS, 0, stream>>>(d_gene, d_first, in, n, sorted_gene, prefix);
    }
    int rc = scan_in_place(ctx, prefix, n, sums, stream);
    if (rc != PGX_OK) return rc;
    {
        ProfScope prof(ctx, "prox_rank_kernel", stream);
        prox_rank_kernel<<<flat_blocks, PX_THREADS, 0, stream>>>(d_first, in, n, sorted_gene, prefix, d_variant, d_distinct);
    }
    {
        ProfScope prof(ctx, "prox_variant_kernel", stream);
        prox_variant_kernel<<<flat_blocks, PX_THREADS, 0, stream>>>(d_first, n, d_variant);
    }
    PGX_HIP(hipGetLastError());
    return PGX_OK;
}

int group_dev(pgx_ctx *ctx, const uint8_t *d_blob, const u64 *d_offsets, const int32_t *d_gene, uint32_t n, uint32_t flags,
              int32_t *d_first, int32_t *d_variant, uint32_t *d_distinct, void *d_ws, size_t ws_bytes, hipStream_t stream) {
    int rc = group_sizes(ctx, n, flags);
    if (rc != PGX_OK) return rc;
    PGX_REQUIRE(d_distinct, "NULL n_distinct");
    PGX_REQUIRE(((uintptr_t)d_distinct & 3u) == 0, "n_distinct must be 4-byte aligned");
    if (n == 0) {
        PGX_HIP(hipMemsetAsync(d_distinct, 0, 4, stream));
        PGX_HIP(hipStreamSynchronize(stream));
        return PGX_OK;
    }
    PGX_REQUIRE(d_blob && d_offsets && d_gene && d_first && d_variant, "NULL argument");
    PGX_REQUIRE(d_ws && ws_bytes >= group_layout(n).bytes, "workspace too small (see pgx_prox_group_workspace_bytes)");
    PGX_REQUIRE(((uintptr_t)d_ws & 15u) == 0, "workspace must be 16-byte aligned");
    PGX_REQUIRE(((uintptr_t)d_offsets & 7u) == 0, "offsets must be 8-byte aligned");
    PGX_REQUIRE((((uintptr_t)d_gene | (uintptr_t)d_first | (uintptr_t)d_variant) & 3u) == 0,
                "gene, first and variant must be 4-byte aligned");
    rc = group_launch(ctx, d_blob, d_offsets, d_gene, n, flags, d_first, d_variant, d_distinct, (uint8_t *)d_ws, stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(hipStreamSynchronize(stream));
    return PGX_OK;
}

int group_host(pgx_ctx *ctx, const uint8_t *blob, const uint64_t *offsets, const int32_t *gene, uint32_t n, uint32_t flags,
               int32_t *out_first, int32_t *out_variant, uint32_t *out_distinct) {
    int rc = group_sizes(ctx, n, flags);
    if (rc != PGX_OK) return rc;
    PGX_REQUIRE(offsets && out_distinct, "NULL offsets or n_distinct");
    for (uint32_t i = 0; i < n; ++i) {
        PGX_REQUIRE(offsets[i] <= offsets[i + 1], "offsets must not decrease");
        PGX_REQUIRE(gene && gene[i] >= 0 && (uint32_t)gene[i] < PX_MAX_GENE, "a gene must lie in [0, 2^24)");
    }
    PGX_REQUIRE(offsets[n] < (1ull << 32), "a blob must hold fewer than 2^32 bytes");
    PGX_REQUIRE(offsets[n] == 0 || blob, "NULL blob");
    if (n == 0) {
        *out_distinct = 0;
        return PGX_OK;
    }
    PGX_REQUIRE(out_first && out_variant, "NULL argument");
    PGX_HIP(hipSetDevice(ctx->device_id));
    DevBuf d_blob(ctx, PX_SLOT_BLOB), d_ws(ctx, PX_SLOT_WS);
    DevPack in(ctx, PX_SLOT_RECORDS), res(ctx, PX_SLOT_RESULT);
    const size_t bytes = (size_t)offsets[n];
    const PackPart i_off = in.in(offsets, (size_t)n + 1), i_gene = in.in(gene, n);
    const PackPart r_first = res.out(out_first, n), r_variant = res.out(out_variant, n), r_distinct = res.out(out_distinct, 1);
    PGX_HIP(d_blob.alloc(bytes));
    PGX_HIP(in.alloc());
    PGX_HIP(res.alloc());
    PGX_HIP(d_ws.alloc(group_layout(n).bytes));
    if (bytes) {
        rc = pgx_staged_h2d(ctx, d_blob.p, blob, bytes, ctx->stream);
        if (rc != PGX_OK) return rc;
    }
    PGX_HIP(in.upload(ctx->stream));
    rc = group_launch(ctx, d_blob.as<uint8_t>(), in.dev<u64>(i_off), in.dev<int32_t>(i_gene), n, flags, res.dev<int32_t>(r_first),
                      res.dev<int32_t>(r_variant), res.dev<uint32_t>(r_distinct), d_ws.as<uint8_t>(), ctx->stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(res.download(ctx->stream));
    PGX_HIP(hipStreamSynchronize(ctx->stream));
    return PGX_OK;
}

}  // namespace

extern "C" {

uint32_t pgx_prox_cut_group_bytes(void) { return PX_STEP; }

uint32_t pgx_prox_group_tile(void) { return PX_TILE; }

size_t pgx_prox_group_workspace_bytes(uint32_t n) {
    if (n >= PX_MAX_N) return 0;
    return group_layout(n).bytes;
}

int pgx_prox_cut(pgx_ctx *ctx, const uint8_t *text, uint64_t text_bytes, const uint64_t *start, const uint32_t *length,
                 const uint8_t *reverse, uint32_t n, uint8_t *out, uint8_t *out_bad) {
    return guarded(__func__, [&] { return cut_host(ctx, text, text_bytes, start, length, reverse, n, out, out_bad); });
}

int pgx_prox_cut_dev(pgx_ctx *ctx, const uint8_t *d_text, uint64_t text_bytes, const uint64_t *d_start,
                     const uint32_t *d_length, const uint8_t *d_reverse, const uint64_t *d_out_offsets, uint32_t n,
                     uint8_t *d_out, uint8_t *d_bad, void *stream) {
    return guarded(__func__, [&] {
        return cut_dev(ctx, d_text, text_bytes, (const u64 *)d_start, d_length, d_reverse, (const u64 *)d_out_offsets, n, d_out,
                       d_bad, (hipStream_t)stream);
    });
}

int pgx_prox_group(pgx_ctx *ctx, const uint8_t *blob, const uint64_t *offsets, const int32_t *gene, uint32_t n,
                   uint32_t flags, int32_t *out_first, int32_t *out_variant, uint32_t *out_n_distinct) {
    return guarded(__func__,
                   [&] { return group_host(ctx, blob, offsets, gene, n, flags, out_first, out_variant, out_n_distinct); });
}

int pgx_prox_group_dev(pgx_ctx *ctx, const uint8_t *d_blob, const uint64_t *d_offsets, const int32_t *d_gene, uint32_t n,
                       uint32_t flags, int32_t *d_first, int32_t *d_variant, uint32_t *d_n_distinct, void *d_workspace,
                       size_t workspace_bytes, void *stream) {
    return guarded(__func__, [&] {
        return group_dev(ctx, d_blob, (const u64 *)d_offsets, d_gene, n, flags, d_first, d_variant, d_n_distinct, d_workspace,
                         workspace_bytes, (hipStream_t)stream);
    });
}

}  // extern "C"
