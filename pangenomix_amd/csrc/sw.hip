// Smith-Waterman with affine gaps on BLOSUM62 for a list of (query, subject) pairs, with the statistics of the best local
// alignment carried through the recurrence instead of a traceback (the primitive behind pangenomix_amd.ncbi.bidirectional_blast;
// the rules are DESIGN.md 6t and pgx.h "Local alignment of pairs"):
//   E[i][j] = max(E[i][j-1] - 1, H[i][j-1] - 12)        F[i][j] = max(F[i-1][j] - 1, H[i-1][j] - 12)
//   H[i][j] = max(0, H[i-1][j-1] + sub(q[i], s[j]), E[i][j], F[i][j])
// On equal values the alternative written first wins; the result of a pair is the cell of maximum H, ties to the smallest i,
// then the smallest j. Every H, E and F carries (q_start, s_start, n_ident, n_cols, n_gapopen) of the path it was chosen from,
// so a cell is a pure function of its three predecessors and the order of evaluation is free.
//
// Mapping: one pair per DPP row of 16 lanes, four pairs per wave, sixteen per workgroup. The query is cut into strips of
// SW_W = 64 positions; lane g of the row owns the SW_CPL = 4 consecutive query positions 4g .. 4g+3 of the strip and keeps
// H[i][j-1] and E[i][j-1] of each in registers. The subject streams through the row: on step t lane g is at subject position
// j = t - g, so what it needs from query position i-1 (H and F at j, and H at j-1 for the diagonal) is what lane g-1 left on
// the step before: one row_shr:1 each. Lane 0 takes them from the strip before, lane 15 leaves them for the next strip:
// a strip's last row goes to the lane group's own piece of the workspace, 16 subject positions at a time -- the 16 lanes load
// (store) positions tb .. tb+15 together and a register rotates through the row by row_shl:1, one position per step, so
// there is one coalesced access per 16 steps and none on the steps' chain. The subject's letters travel the same way, and
// the query's letters are four bytes per lane and strip: neither sequence needs LDS, which holds only the substitution
// table over letters (27 x 32 entries: A-Z and one class for everything else).
//
// Kernels (plain launches on one stream, no atomics: a pair is owned by one lane group and written by one lane):
//   sw_kernel<false>   H, E, F and the best cell of every pair: out = {score, 0, q_end, 0, s_end, 0, 0, 0}
//   sw_compact_kernel  one workgroup: the slots whose pair has score >= min_score and score > 0, in slot order (a count and an
//                      exclusive scan over contiguous chunks)
//   sw_kernel<true>    the same recurrence with the carried statistics (three dwords: q_start << 16 | s_start,
//                      n_ident << 16 | n_cols, n_gapopen) over those slots: all eight values
#include "pgx_internal.h"
#include "cluster_tables.h"

#include <numeric>

namespace {

using u64 = unsigned long long;

constexpr int SW_CPL = 4;                        // query positions per lane
constexpr int SW_W = 16 * SW_CPL;                // ... and per strip
constexpr uint32_t SW_MAX_LEN = 4096;            // positions and column counts stay below 2^16 (n_cols <= 2 * SW_MAX_LEN)
constexpr int SW_THREADS = 256;                  // 16 lane groups
constexpr int SW_GROUPS = SW_THREADS / 16;
constexpr int SW_OPEN = 12, SW_EXT = 1;          // a gap of k residues costs 11 + k
constexpr int SW_NEG = -(1 << 29);               // minus infinity: never decremented more than once before a max with >= -12
constexpr int SW_LETTERS = 27, SW_TAB_STRIDE = 32;
constexpr uint32_t SW_WG_PER_CU_SCORE = 8, SW_WG_PER_CU_STATS = 2;   // the workspace grows with either
constexpr int SW_COMPACT_THREADS = 1024;
constexpr uint32_t SW_BAD_PAIR = 1u;             // status bit: an index, an offset or a length a kernel refused
constexpr size_t SW_HEAD_BYTES = 32;             // the workspace's head: status, then the compacted count (16 bytes each)

struct SubTable { int8_t v[SW_LETTERS * SW_TAB_STRIDE]; };

// substitution score of two letters (A-Z = 0..25, 26 = anything else), through the 21 classes of cluster_tables.h
SubTable make_sub_table() {
    SubTable t{};
    for (int a = 0; a < SW_LETTERS; ++a)
        for (int b = 0; b < SW_LETTERS; ++b) {
            const int ca = a < 26 ? pgxc::kAa2Idx[a] : 20, cb = b < 26 ? pgxc::kAa2Idx[b] : 20;
            t.v[a * SW_TAB_STRIDE + b] = pgxc::kBlosum62[ca][cb];
        }
    return t;
}

__host__ __device__ __forceinline__ uint32_t sw_letter(uint32_t byte) {
    const uint32_t u = (byte | 32u) - (uint32_t)'a';
    return u < 26u ? u : 26u;
}

// dwords of workspace per subject position of one lane group: H and F of a strip's last row, and their statistics
template <bool STATS> constexpr uint32_t sw_bnd_dwords() { return STATS ? 8u : 2u; }

// lane g takes lane g-1's `v`; lane 0 of a row keeps `first`
__device__ __forceinline__ int shr1_or(int first, int v) { return __builtin_amdgcn_update_dpp(first, v, 0x111, 0xF, 0xF, false); }
// lane g takes lane g+1's `v`; lane 15 of a row keeps `last`
__device__ __forceinline__ int shl1_or(int last, int v) { return __builtin_amdgcn_update_dpp(last, v, 0x101, 0xF, 0xF, false); }

struct Stat {               // of a path: q_start << 16 | s_start, n_ident << 16 | n_cols, n_gapopen
    uint32_t a, b, c;
};
__device__ __forceinline__ Stat stat_pick(bool first, const Stat &x, const Stat &y) {
    return Stat{first ? x.a : y.a, first ? x.b : y.b, first ? x.c : y.c};
}
__device__ __forceinline__ Stat stat_shr1_or(const Stat &first, const Stat &v) {
    return Stat{(uint32_t)shr1_or((int)first.a, (int)v.a), (uint32_t)shr1_or((int)first.b, (int)v.b),
                (uint32_t)shr1_or((int)first.c, (int)v.c)};
}
__device__ __forceinline__ Stat stat_shl1_or(const Stat &last, const Stat &v) {
    return Stat{(uint32_t)shl1_or((int)last.a, (int)v.a), (uint32_t)shl1_or((int)last.b, (int)v.b),
                (uint32_t)shl1_or((int)last.c, (int)v.c)};
}

template <bool STATS>
__global__ __launch_bounds__(SW_THREADS) void sw_kernel(const uint8_t *__restrict__ res1, const u64 *__restrict__ off1, uint32_t n1,
                                                        const uint8_t *__restrict__ res2, const u64 *__restrict__ off2, uint32_t n2,
                                                        const uint32_t *__restrict__ pair_a, const uint32_t *__restrict__ pair_b,
                                                        const uint32_t *__restrict__ list, const uint32_t *__restrict__ n_list,
                                                        uint32_t n_slots, uint32_t max_len, SubTable sub, int32_t *bnd_all,
                                                        int32_t *__restrict__ out, uint32_t *status) {
    constexpr uint32_t DW = sw_bnd_dwords<STATS>();
    __shared__ int tab[SW_LETTERS * SW_TAB_STRIDE];
    if (n_list) n_slots = *n_list;
    if (blockIdx.x * (uint32_t)SW_GROUPS >= n_slots) return;
    // with statistics: score * 2 + (the same letter)
    for (int c = threadIdx.x; c < SW_LETTERS * SW_TAB_STRIDE; c += SW_THREADS)
        tab[c] = STATS ? (int)sub.v[c] * 2 + (c / SW_TAB_STRIDE == c % SW_TAB_STRIDE ? 1 : 0) : (int)sub.v[c];
    __syncthreads();
    const int g = threadIdx.x & 15;
    const uint32_t group = threadIdx.x >> 4;
    int32_t *bnd = bnd_all + ((size_t)blockIdx.x * SW_GROUPS + group) * (size_t)max_len * DW;

    for (uint32_t base = blockIdx.x * (uint32_t)SW_GROUPS; base < n_slots; base += gridDim.x * (uint32_t)SW_GROUPS) {
        const uint32_t slot = base + group;
        if (slot >= n_slots) continue;                                           // (the whole lane group)
        const uint32_t p = list ? list[slot] : slot;
        const uint32_t ia = pair_a[p], ib = pair_b[p];
        int32_t *o = out + (size_t)p * 8;
        u64 q0 = 0, s0 = 0, m64 = 0, n64 = 0;
        bool ok = ia < n1 && ib < n2;
        if (ok) {
            q0 = off1[ia]; s0 = off2[ib];
            const u64 q1 = off1[ia + 1], s1 = off2[ib + 1];
            ok = q1 >= q0 && s1 >= s0 && q1 - q0 <= max_len && s1 - s0 <= max_len;
            m64 = q1 - q0; n64 = s1 - s0;
        }
        if (!ok || m64 == 0 || n64 == 0) {                                       // an empty sequence: score 0 at (0, 0)
            if (g < 8) o[g] = 0;
            if (!ok && g == 0) *status = SW_BAD_PAIR;                            // (every writer stores the same word)
            continue;
        }
        const int m = (int)m64, n = (int)n64;
        const uint8_t *q = res1 + q0, *s = res2 + s0;
        u64 best = 0;                                                            // H << 32 | ~(i << 16 | j): max = the rule's cell
        Stat best_st{0, 0, 0};

        for (int i_strip = 0; i_strip < m; i_strip += SW_W) {
            const bool first_strip = i_strip == 0, last_strip = i_strip + SW_W >= m;
            const int i0 = i_strip + g * SW_CPL;
            int qrow[SW_CPL];
            uint32_t live[SW_CPL], not_i[SW_CPL];
#pragma unroll
            for (int c = 0; c < SW_CPL; ++c) {
                const int i = i0 + c;
                qrow[c] = (int)(i < m ? sw_letter(q[i]) : 26u) * SW_TAB_STRIDE;
                live[c] = i < m ? 0xFFFFFFFFu : 0u;
                not_i[c] = ~((uint32_t)i << 16);
            }
            int Hp[SW_CPL], Ep[SW_CPL];                                          // H[i][j-1], E[i][j-1]
            Stat Hs[SW_CPL], Es[SW_CPL];
#pragma unroll
            for (int c = 0; c < SW_CPL; ++c) { Hp[c] = 0; Ep[c] = SW_NEG; Hs[c] = Stat{0, 0, 0}; Es[c] = Stat{0, 0, 0}; }
            int lastF = SW_NEG;                                                  // F of the lane's last position (H is Hp[SW_CPL-1])
            Stat lastFs{0, 0, 0};
            int upH_before = 0;                                                  // H[i0-1][j-1]
            Stat upHs_before{0, 0, 0};
            int s_here = 0;
            int outH = 0, outF = 0;
            Stat outHs{0, 0, 0}, outFs{0, 0, 0};

            for (int tb = 0; tb < n + 15; tb += 16) {
                // ---- what lane 0 will take on the next 16 steps: the subject's letters and the strip before ----
                const int jf = tb + g;
                int feed_s = jf < n ? (int)sw_letter(s[jf]) : 26;
                int feedH = 0, feedF = SW_NEG;
                Stat feedHs{0, 0, 0}, feedFs{0, 0, 0};
                if (!first_strip && jf < n) {
                    if constexpr (STATS) {
                        const int4 x = *reinterpret_cast<const int4 *>(bnd + (size_t)jf * DW);
                        const int4 y = *reinterpret_cast<const int4 *>(bnd + (size_t)jf * DW + 4);
                        feedH = x.x; feedF = x.y;
                        feedHs = Stat{(uint32_t)x.z, (uint32_t)x.w, (uint32_t)y.x};
                        feedFs = Stat{(uint32_t)y.y, (uint32_t)y.z, (uint32_t)y.w};
                    } else {
                        const int2 x = *reinterpret_cast<const int2 *>(bnd + (size_t)jf * DW);
                        feedH = x.x; feedF = x.y;
                    }
                }
#pragma unroll 4
                for (int k = 0; k < 16; ++k) {
                    const int j = tb + k - g;
                    // from query position i0 - 1: lane g-1's last position on the step before, or the strip before
                    int upH = shr1_or(feedH, Hp[SW_CPL - 1]);
                    int upF = shr1_or(feedF, lastF);
                    Stat upHs{0, 0, 0}, upFs{0, 0, 0};
                    if constexpr (STATS) {
                        upHs = stat_shr1_or(feedHs, Hs[SW_CPL - 1]);
                        upFs = stat_shr1_or(feedFs, lastFs);
                    }
                    s_here = shr1_or(feed_s, s_here);
                    const int upH_in = upH;
                    const Stat upHs_in = upHs;
                    if ((unsigned)j < (unsigned)n) {
                        int diag = upH_before;
                        Stat diag_s = upHs_before;
#pragma unroll
                        for (int c = 0; c < SW_CPL; ++c) {
                            const int tv = tab[qrow[c] + s_here];
                            const int e_ext = Ep[c] - SW_EXT, e_open = Hp[c] - SW_OPEN;
                            const int f_ext = upF - SW_EXT, f_open = upH - SW_OPEN;
                            const int E = max(e_ext, e_open), F = max(f_ext, f_open);
                            int H;
                            Stat hs{0, 0, 0}, es{0, 0, 0}, fs{0, 0, 0};
                            if constexpr (STATS) {
                                const int d = diag + (tv >> 1);
                                const uint32_t same = (uint32_t)(tv & 1);
                                es = stat_pick(e_ext >= e_open, Stat{Es[c].a, Es[c].b + 1u, Es[c].c}, Stat{Hs[c].a, Hs[c].b + 1u, Hs[c].c + 1u});
                                fs = stat_pick(f_ext >= f_open, Stat{upFs.a, upFs.b + 1u, upFs.c}, Stat{upHs.a, upHs.b + 1u, upHs.c + 1u});
                                const uint32_t here = ((uint32_t)(i0 + c) << 16) | (uint32_t)j;
                                const Stat ds = stat_pick(diag == 0, Stat{here, (same << 16) + 1u, 0u},
                                                          Stat{diag_s.a, diag_s.b + (same << 16) + 1u, diag_s.c});
                                H = d; hs = ds;
                                hs = stat_pick(E > H, es, hs); H = max(H, E);
                                hs = stat_pick(F > H, fs, hs); H = max(H, F);
                                H = max(H, 0);
                            } else {
                                H = max(max(diag + tv, 0), max(E, F));
                            }
                            const u64 key = ((u64)((uint32_t)H & live[c]) << 32) | (u64)(not_i[c] - (uint32_t)j);
                            const bool better = key > best;
                            best = better ? key : best;
                            if constexpr (STATS) best_st = stat_pick(better, hs, best_st);
                            diag = Hp[c]; diag_s = Hs[c];                        // H[i][j-1]: the diagonal of position i + 1
                            Hp[c] = H; Ep[c] = E; Hs[c] = hs; Es[c] = es;
                            upH = H; upF = F; upHs = hs; upFs = fs;
                        }
                        lastF = upF; lastFs = upFs;
                    }
                    upH_before = upH_in; upHs_before = upHs_in;
                    // rotate: lane 0 sees the next position's feed, lane 15's last row moves towards the lane that stores it
                    feed_s = shl1_or(0, feed_s);
                    feedH = shl1_or(0, feedH); feedF = shl1_or(0, feedF);
                    outH = shl1_or(Hp[SW_CPL - 1], outH); outF = shl1_or(lastF, outF);
                    if constexpr (STATS) {
                        feedHs = stat_shl1_or(Stat{0, 0, 0}, feedHs); feedFs = stat_shl1_or(Stat{0, 0, 0}, feedFs);
                        outHs = stat_shl1_or(Hs[SW_CPL - 1], outHs); outFs = stat_shl1_or(lastFs, outFs);
                    }
                }
                // ---- lane g holds lane 15's last row of step tb + g, which is subject position tb + g - 15 ----
                const int jo = tb + g - 15;
                if (!last_strip && jo >= 0 && jo < n) {
                    if constexpr (STATS) {
                        *reinterpret_cast<int4 *>(bnd + (size_t)jo * DW) = make_int4(outH, outF, (int)outHs.a, (int)outHs.b);
                        *reinterpret_cast<int4 *>(bnd + (size_t)jo * DW + 4) = make_int4((int)outHs.c, (int)outFs.a, (int)outFs.b, (int)outFs.c);
                    } else {
                        *reinterpret_cast<int2 *>(bnd + (size_t)jo * DW) = make_int2(outH, outF);
                    }
                }
            }
            // the next strip's lanes read what other lanes of this row stored
            __threadfence_block();
        }
        // ---- the row's best cell: the key is different in every cell, so the maximum is one cell's ----
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) {
            const u64 other = __shfl_xor(best, d, 16);
            const bool take = other > best;
            if constexpr (STATS) {
                const uint32_t oa = (uint32_t)__shfl_xor((int)best_st.a, d, 16), ob = (uint32_t)__shfl_xor((int)best_st.b, d, 16),
                               oc = (uint32_t)__shfl_xor((int)best_st.c, d, 16);
                best_st = stat_pick(take, Stat{oa, ob, oc}, best_st);
            }
            best = take ? other : best;
        }
        if (g == 0) {
            const int score = (int)(best >> 32);
            const uint32_t pos = ~(uint32_t)best;
            const bool with = STATS && score > 0;
            o[0] = score;
            o[1] = with ? (int)(best_st.a >> 16) : 0;
            o[2] = (int)(pos >> 16);
            o[3] = with ? (int)(best_st.a & 0xFFFFu) : 0;
            o[4] = (int)(pos & 0xFFFFu);
            o[5] = with ? (int)(best_st.b >> 16) : 0;
            o[6] = with ? (int)(best_st.b & 0xFFFFu) : 0;
            o[7] = with ? (int)best_st.c : 0;
        }
    }
}

// list_out = the slots (in order) whose pair reached its min_score with a positive score; *n_out = how many. One workgroup.
__global__ __launch_bounds__(SW_COMPACT_THREADS) void sw_compact_kernel(const uint32_t *__restrict__ list, uint32_t n_slots,
                                                                        const int32_t *__restrict__ min_score,
                                                                        const int32_t *__restrict__ out,
                                                                        uint32_t *__restrict__ list_out, uint32_t *__restrict__ n_out) {
    __shared__ uint32_t counts[SW_COMPACT_THREADS];
    const uint32_t tid = threadIdx.x;
    const uint32_t chunk = (n_slots + SW_COMPACT_THREADS - 1) / SW_COMPACT_THREADS;
    const uint32_t begin = min(n_slots, tid * chunk), end = min(n_slots, begin + chunk);
    auto wanted = [&](uint32_t slot, uint32_t &p) {
        p = list ? list[slot] : slot;
        const int32_t score = out[(size_t)p * 8];
        return score > 0 && score >= min_score[p];
    };
    uint32_t mine = 0, p;
    for (uint32_t i = begin; i < end; ++i) mine += wanted(i, p) ? 1u : 0u;
    counts[tid] = mine;
    __syncthreads();
    for (uint32_t d = 1; d < SW_COMPACT_THREADS; d <<= 1) {                      // inclusive scan
        const uint32_t v = tid >= d ? counts[tid - d] : 0u;
        __syncthreads();
        counts[tid] += v;
        __syncthreads();
    }
    uint32_t at = counts[tid] - mine;
    for (uint32_t i = begin; i < end; ++i)
        if (wanted(i, p)) list_out[at++] = p;
    if (tid == SW_COMPACT_THREADS - 1) *n_out = counts[tid];
}

// the most workgroups a pass launches: beyond them a lane group takes a further pair per round of the grid
uint32_t sw_grid_cap(pgx_ctx *ctx, uint32_t per_cu) {
    const uint32_t cus = ctx->prop.multiProcessorCount > 0 ? (uint32_t)ctx->prop.multiProcessorCount : 1u;
    return cus * per_cu;
}

uint32_t sw_grid(pgx_ctx *ctx, uint32_t n_pairs, uint32_t per_cu) {
    return std::max(1u, std::min(ceil_div_u32(n_pairs, SW_GROUPS), sw_grid_cap(ctx, per_cu)));
}

// head | the compacted list | the strips' last rows of either pass (the passes run one after the other)
struct SwLayout {
    size_t off_list, off_bnd, bytes;
};
SwLayout sw_layout(pgx_ctx *ctx, uint32_t n_pairs, uint32_t max_len) {
    WsLayout lay;
    lay.take(SW_HEAD_BYTES);
    SwLayout L{};
    L.off_list = lay.take((size_t)n_pairs * 4);
    const size_t score = (size_t)sw_grid(ctx, n_pairs, SW_WG_PER_CU_SCORE) * SW_GROUPS * max_len * sw_bnd_dwords<false>() * 4;
    const size_t stats = (size_t)sw_grid(ctx, n_pairs, SW_WG_PER_CU_STATS) * SW_GROUPS * max_len * sw_bnd_dwords<true>() * 4;
    L.off_bnd = lay.take(std::max(score, stats));
    L.bytes = lay.total();
    return L;
}

// Both passes, enqueued on `stream`; then `stream` is synchronised and the status word read. d_order: the slots' pairs, or NULL.
int sw_run(pgx_ctx *ctx, const uint8_t *d_res1, const u64 *d_off1, uint32_t n1, const uint8_t *d_res2, const u64 *d_off2,
           uint32_t n2, const uint32_t *d_a, const uint32_t *d_b, uint32_t n_pairs, const int32_t *d_min, const uint32_t *d_order,
           uint32_t max_len, int32_t *d_out, void *d_ws, hipStream_t stream) {
    static const SubTable sub = make_sub_table();
    const SwLayout L = sw_layout(ctx, n_pairs, max_len);
    char *ws = static_cast<char *>(d_ws);
    uint32_t *d_status = reinterpret_cast<uint32_t *>(ws), *d_count = reinterpret_cast<uint32_t *>(ws + 16);
    uint32_t *d_list = reinterpret_cast<uint32_t *>(ws + L.off_list);
    int32_t *d_bnd = reinterpret_cast<int32_t *>(ws + L.off_bnd);
    PGX_HIP(hipMemsetAsync(ws, 0, SW_HEAD_BYTES, stream));
    {
        ProfScope prof(ctx, "sw_score_kernel", stream);
        sw_kernel<false><<<sw_grid(ctx, n_pairs, SW_WG_PER_CU_SCORE), SW_THREADS, 0, stream>>>(
            d_res1, d_off1, n1, d_res2, d_off2, n2, d_a, d_b, d_order, nullptr, n_pairs, max_len, sub, d_bnd, d_out, d_status);
    }
    PGX_HIP(hipGetLastError());
    {
        ProfScope prof(ctx, "sw_compact_kernel", stream);
        sw_compact_kernel<<<1, SW_COMPACT_THREADS, 0, stream>>>(d_order, n_pairs, d_min, d_out, d_list, d_count);
    }
    PGX_HIP(hipGetLastError());
    {
        ProfScope prof(ctx, "sw_stats_kernel", stream);
        sw_kernel<true><<<sw_grid(ctx, n_pairs, SW_WG_PER_CU_STATS), SW_THREADS, 0, stream>>>(
            d_res1, d_off1, n1, d_res2, d_off2, n2, d_a, d_b, d_list, d_count, n_pairs, max_len, sub, d_bnd, d_out, d_status);
    }
    PGX_HIP(hipGetLastError());
    uint32_t head[8] = {};
    PGX_HIP(hipMemcpyAsync(head, ws, SW_HEAD_BYTES, hipMemcpyDeviceToHost, stream));
    PGX_HIP(hipStreamSynchronize(stream));
    PGX_REQUIRE(head[0] == 0, "a pair names a sequence that does not exist, offsets decrease, or a sequence is longer than max_len");
    ctx->sw_stats_pairs = head[4];
    return PGX_OK;
}

int sw_pairs_dev(pgx_ctx *ctx, const uint8_t *d_res1, const u64 *d_off1, uint32_t n1, const uint8_t *d_res2, const u64 *d_off2,
                 uint32_t n2, const uint32_t *d_a, const uint32_t *d_b, uint32_t n_pairs, const int32_t *d_min, uint32_t max_len,
                 int32_t *d_out, void *d_ws, size_t ws_bytes, hipStream_t stream) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(max_len >= 1 && max_len <= SW_MAX_LEN, "max_len must be 1..pgx_sw_max_length()");
    PGX_REQUIRE(n_pairs < (1u << 30), "n_pairs must be below 2^30");
    if (n_pairs == 0) return PGX_OK;
    PGX_REQUIRE(d_res1 && d_off1 && d_res2 && d_off2 && d_a && d_b && d_min && d_out, "NULL argument");
    PGX_REQUIRE(((uintptr_t)d_off1 & 7u) == 0 && ((uintptr_t)d_off2 & 7u) == 0, "offsets must be 8-byte aligned");
    PGX_REQUIRE(((uintptr_t)d_a & 3u) == 0 && ((uintptr_t)d_b & 3u) == 0 && ((uintptr_t)d_min & 3u) == 0 && ((uintptr_t)d_out & 3u) == 0,
                "pair_a, pair_b, min_score and out must be 4-byte aligned");
    PGX_REQUIRE(d_ws && ws_bytes >= sw_layout(ctx, n_pairs, max_len).bytes, "workspace too small (see pgx_sw_workspace_bytes)");
    PGX_REQUIRE(((uintptr_t)d_ws & 15u) == 0, "workspace must be 16-byte aligned");
    return sw_run(ctx, d_res1, d_off1, n1, d_res2, d_off2, n2, d_a, d_b, n_pairs, d_min, nullptr, max_len, d_out, d_ws, stream);
}

const char *sw_offsets_error(const uint64_t *off, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return "offsets must not decrease";
    return off[0] == 0 ? nullptr : "offsets must begin with 0";
}

int sw_pairs_host(pgx_ctx *ctx, const uint8_t *res1, const uint64_t *off1, uint32_t n1, const uint8_t *res2, const uint64_t *off2,
                  uint32_t n2, const uint32_t *pair_a, const uint32_t *pair_b, uint32_t n_pairs, const int32_t *min_score,
                  int32_t *out) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(n_pairs < (1u << 30), "n_pairs must be below 2^30");
    if (n_pairs == 0) return PGX_OK;
    PGX_REQUIRE(off1 && off2 && pair_a && pair_b && min_score && out, "NULL argument");
    const char *broken = sw_offsets_error(off1, n1);
    if (!broken) broken = sw_offsets_error(off2, n2);
    PGX_REQUIRE(!broken, broken);
    PGX_REQUIRE((off1[n1] == 0 || res1) && (off2[n2] == 0 || res2), "NULL residues");
    // the pairs by steps of the kernel, longest first: the four rows of a wave and the waves of a workgroup finish together,
    // and the grid's last round is its shortest
    std::vector<uint32_t> order(n_pairs);
    std::vector<uint64_t> steps(n_pairs);
    uint32_t max_len = 1;
    for (uint32_t p = 0; p < n_pairs; ++p) {
        PGX_REQUIRE(pair_a[p] < n1 && pair_b[p] < n2, "a pair names a sequence that does not exist");
        const uint64_t m = off1[pair_a[p] + 1] - off1[pair_a[p]], n = off2[pair_b[p] + 1] - off2[pair_b[p]];
        PGX_REQUIRE(m <= SW_MAX_LEN && n <= SW_MAX_LEN, "a sequence of a pair is longer than pgx_sw_max_length()");
        max_len = std::max(max_len, (uint32_t)std::max(m, n));
        steps[p] = ((m + SW_W - 1) / SW_W) * ((n + 15 + 15) / 16);
    }
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return steps[x] > steps[y]; });
    PGX_HIP(hipSetDevice(ctx->device_id));
    hipStream_t stream = ctx->stream;
    DevBuf d_res1(ctx, SW_SLOT_RES1), d_res2(ctx, SW_SLOT_RES2), d_ws(ctx, SW_SLOT_WS);
    DevPack in(ctx, SW_SLOT_IN), res(ctx, SW_SLOT_OUT);
    const PackPart p_off1 = in.in(off1, (size_t)n1 + 1), p_off2 = in.in(off2, (size_t)n2 + 1);
    const PackPart p_a = in.in(pair_a, n_pairs), p_b = in.in(pair_b, n_pairs), p_min = in.in(min_score, n_pairs);
    const PackPart p_order = in.in(order.data(), n_pairs);
    const PackPart p_out = res.out(out, (size_t)n_pairs * 8);
    PGX_HIP(d_res1.alloc((size_t)off1[n1]));
    PGX_HIP(d_res2.alloc((size_t)off2[n2]));
    PGX_HIP(d_ws.alloc(sw_layout(ctx, n_pairs, max_len).bytes));
    PGX_HIP(in.alloc());
    PGX_HIP(res.alloc());
    int rc = pgx_staged_h2d(ctx, d_res1.p, res1, (size_t)off1[n1], stream);
    if (rc != PGX_OK) return rc;
    rc = pgx_staged_h2d(ctx, d_res2.p, res2, (size_t)off2[n2], stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(in.upload(stream));
    rc = sw_run(ctx, d_res1.as<uint8_t>(), in.dev<u64>(p_off1), n1, d_res2.as<uint8_t>(), in.dev<u64>(p_off2), n2,
                in.dev<uint32_t>(p_a), in.dev<uint32_t>(p_b), n_pairs, in.dev<int32_t>(p_min), in.dev<uint32_t>(p_order), max_len,
                res.dev<int32_t>(p_out), d_ws.p, stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(res.download(stream));
    PGX_HIP(hipStreamSynchronize(stream));
    return PGX_OK;
}

}  // namespace

extern "C" {

uint32_t pgx_sw_max_length(void) { return SW_MAX_LEN; }

uint32_t pgx_sw_strip_width(void) { return SW_W; }

size_t pgx_sw_workspace_bytes(pgx_ctx *ctx, uint32_t n_pairs, uint32_t max_len) {
    if (!ctx || max_len < 1 || max_len > SW_MAX_LEN || n_pairs >= (1u << 30)) return 0;
    return sw_layout(ctx, n_pairs, max_len).bytes;
}

uint32_t pgx_sw_last_stats_pairs(pgx_ctx *ctx) { return ctx ? ctx->sw_stats_pairs : 0; }

uint32_t pgx_sw_round_pairs(pgx_ctx *ctx, int with_stats) {
    return ctx ? sw_grid_cap(ctx, with_stats ? SW_WG_PER_CU_STATS : SW_WG_PER_CU_SCORE) * (uint32_t)SW_GROUPS : 0;
}

int pgx_sw_pairs(pgx_ctx *ctx, const uint8_t *residues1, const uint64_t *offsets1, uint32_t n1, const uint8_t *residues2,
                 const uint64_t *offsets2, uint32_t n2, const uint32_t *pair_a, const uint32_t *pair_b, uint32_t n_pairs,
                 const int32_t *min_score, int32_t *out) {
    return guarded(__func__, [&] {
        return sw_pairs_host(ctx, residues1, offsets1, n1, residues2, offsets2, n2, pair_a, pair_b, n_pairs, min_score, out);
    });
}

int pgx_sw_pairs_dev(pgx_ctx *ctx, const uint8_t *d_residues1, const uint64_t *d_offsets1, uint32_t n1, const uint8_t *d_residues2,
                     const uint64_t *d_offsets2, uint32_t n2, const uint32_t *d_pair_a, const uint32_t *d_pair_b, uint32_t n_pairs,
                     const int32_t *d_min_score, uint32_t max_len, int32_t *d_out, void *d_workspace, size_t workspace_bytes,
                     void *stream) {
    return guarded(__func__, [&] {
        return sw_pairs_dev(ctx, d_residues1, (const u64 *)d_offsets1, n1, d_residues2, (const u64 *)d_offsets2, n2, d_pair_a, d_pair_b,
                            n_pairs, d_min_score, max_len, d_out, d_workspace, workspace_bytes, (hipStream_t)stream);
    });
}

}  // extern "C"
