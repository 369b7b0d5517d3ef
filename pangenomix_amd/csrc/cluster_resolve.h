// The host-only logic of a clustering window (plain C++: no HIP, so that a stand-alone program can exercise it;
// tests/cluster_resolve_check.cpp): the records the device and the host share, how a window is formed from the sorted
// lengths, the per-length threshold tables, the in-order walk of a block, and the counting passes over pair records.
// Arguments in, results out; nothing here touches a stream. cluster.hip alternates walk_block with the device's
// follow-up evaluations.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace pgxc {

enum : uint32_t { F_DIAG_PASS = 1, F_BAND_OK = 2, F_ACCEPT = 4, F_TOO_BIG = 8, F_EVAL = 16, F_ALIGNED = 32 };

struct Pair {           // one (query, representative) candidate
    uint32_t q;         // sorted sequence index of the query
    uint32_t r;         // phase A: representative index; phase B: sorted sequence index
    uint32_t cnt;       // short-word count
    uint32_t minc;      // smallest shared word code (candidate order key)
    int32_t best_sum, band_left, band_center, band_right;
    int32_t iden;
    uint32_t flags;
};

// state of a window member on the host (indexed by its position in the window)
enum : uint8_t { ST_OPEN = 0, ST_MEMBER = 1, ST_REP = 2,
                 ST_ABSENT = 3,    // memory-chunked rule: placed by an earlier chunk's sweep, not a member of this window any more
                 ST_NONE = 4 };    // ... a sweep found no representative for it: it stays in the game

constexpr unsigned long long kNoBest = ~0ull;

constexpr uint32_t kMaxChunks = 32;
struct Chunks { uint32_t n; uint32_t begin[kMaxChunks + 1]; };   // member ql belongs to chunk c: begin[c] <= ql < begin[c+1]

// sequences n .. 2n-1 are the reverse complements of 0 .. n-1 (nucleotides, both strands)
inline uint32_t real_seq(uint32_t k, uint32_t n) { return k >= n ? k - n : k; }
// the candidate order of the sequential rule: strand << 63 | smallest shared code << 32 | candidate
inline unsigned long long pair_key(const Pair &p, uint32_t n) {
    return ((unsigned long long)(p.q >= n) << 63) | ((unsigned long long)p.minc << 32) | p.r;
}
inline bool pair_is_aligned(const Pair &p) { return (p.flags & (F_DIAG_PASS | F_BAND_OK)) == (F_DIAG_PASS | F_BAND_OK); }
inline bool pair_band_too_wide(const Pair &p) { return (p.flags & F_TOO_BIG) && (p.flags & F_DIAG_PASS); }

// A window = the members b0 .. b0 + nb - 1 of the sorted list (len[] = their lengths): at most window_cap of them, none
// at or beyond `limit`, in at most kMaxChunks chunks; with `chunking` a chunk closes before its lengths would add up to
// more than chunk_words (or holds one sequence). Returns nb; C.begin[C.n] == nb.
inline uint32_t form_window(const uint32_t *len, uint32_t b0, uint32_t limit, uint32_t window_cap, bool chunking,
                            uint64_t chunk_words, Chunks &C) {
    C.n = 1; C.begin[0] = 0;
    uint64_t in_chunk = 0;
    uint32_t q = 0;
    for (; b0 + q < limit && q < window_cap; ++q) {
        const uint64_t w = len[b0 + q];
        if (chunking && in_chunk && in_chunk + w > chunk_words) {
            if (C.n == kMaxChunks) break;
            C.begin[C.n++] = q;
            in_chunk = 0;
        }
        in_chunk += w;
    }
    C.begin[C.n] = q;
    return q;
}

// per-query thresholds in double, exactly as the sequential rule computes them. They depend on the length only: one
// table of max_len + 1 entries per threshold (identical residues, diagonal hits, shared words).
inline void threshold_tables(double identity, int word_len, double aas_cutoff, double aan_cutoff, bool nt,
                             uint32_t max_len, int32_t *t_aa1, int32_t *t_aas, int32_t *t_aan) {
    for (uint32_t L = 0; L <= max_len; ++L) {
        const int len = (int)L;
        const int aa1 = (int)(identity * (double)len);
        t_aa1[L] = aa1;
        if (identity > 0.95) {
            t_aas[L] = len - (nt ? 4 : 2) + 1 - (len - aa1) * (nt ? 4 : 2);
            t_aan[L] = len - word_len + 1 - (len - aa1) * word_len;
        } else {
            t_aas[L] = (int)(aas_cutoff * (double)len);
            t_aan[L] = (int)(aan_cutoff * (double)len);
        }
    }
}

// A block as the device published it: its members in order, and the candidate pairs between them (q, r = sorted
// sequence indices of members, r before q) bucketed by the query's rank in the block.
struct Block {
    const uint32_t *members;   // [n_members] sorted sequence indices, ascending
    uint32_t n_members;
    const Pair *pairs;         // [n_pairs]
    uint32_t n_pairs;
    uint32_t b0, n;            // first member of the window; sequences per strand
    const uint32_t *bucket;    // [n_members + 1] pairs of member t = order[bucket[t] .. bucket[t + 1])
    const uint32_t *order;     // [n_pairs]
};

// Counting sort of the pairs by the query's rank in the block. rank_of is indexed by the position in the window (only
// the members' entries are written); bucket has n_members + 1 entries, fill n_members, order n_pairs.
inline void bucket_block_pairs(const uint32_t *members, uint32_t n_members, const Pair *pairs, uint32_t n_pairs,
                               uint32_t b0, uint32_t n, uint32_t *rank_of, uint32_t *bucket, uint32_t *fill,
                               uint32_t *order) {
    for (uint32_t t = 0; t < n_members; ++t) { rank_of[members[t] - b0] = t; bucket[t] = 0; }
    bucket[n_members] = 0;
    for (uint32_t i = 0; i < n_pairs; ++i) bucket[rank_of[real_seq(pairs[i].q, n) - b0] + 1]++;
    for (uint32_t t = 0; t < n_members; ++t) bucket[t + 1] += bucket[t];   // bucket t = [bucket[t], bucket[t+1])
    for (uint32_t t = 0; t < n_members; ++t) fill[t] = bucket[t];
    for (uint32_t i = 0; i < n_pairs; ++i) order[fill[rank_of[real_seq(pairs[i].q, n) - b0]]++] = i;
}

enum WalkResult { WALK_DONE = 0,       // every member is decided
                  WALK_OPEN = 1,       // some are not: `flight` lists the pairs to evaluate before the next pass
                  WALK_BAND = 2 };     // an evaluated pair passed the diagonal test with a band the aligner cannot take

// One pass of the in-order walk over the members from rank t_first on. For member q the sequential rule takes the
// accepted representative with the smallest (minc, index) among its in-block candidates that ARE representatives.
// Pairs that have not been evaluated (F_EVAL clear) and that could precede the winner are collected in `flight` for
// ALL still-open members in one pass (candidates that are themselves undecided count as possible representatives);
// the caller has them evaluated and calls again until every member is decided. status and winner_key are indexed by
// the position in the window, iden_of and strand_of by the sorted sequence index. t_first moves past the decided
// members in front.
inline WalkResult walk_block(const Block &B, uint32_t &t_first, uint8_t *status, unsigned long long *winner_key,
                             int32_t *iden_of, uint8_t *strand_of, std::vector<uint32_t> &flight) {
    flight.clear();
    bool any_open = false;
    for (uint32_t t = t_first; t < B.n_members; ++t) {
        const uint32_t k = B.members[t], q = k - B.b0;
        if (status[q] != ST_OPEN) continue;
        const uint32_t lo = B.bucket[t], hi = B.bucket[t + 1];
        unsigned long long win = kNoBest, open_acc = kNoBest;
        int32_t win_iden = 0;
        for (uint32_t e = lo; e < hi; ++e) {
            const Pair &pr = B.pairs[B.order[e]];
            const uint8_t su = status[pr.r - B.b0];
            if (su == ST_MEMBER || !(pr.flags & F_EVAL)) continue;
            if (pair_band_too_wide(pr)) return WALK_BAND;
            if (!(pr.flags & F_ACCEPT)) continue;
            const unsigned long long key = pair_key(pr, B.n);
            if (su == ST_REP) { if (key < win) { win = key; win_iden = pr.iden; } }
            else if (key < open_acc) open_acc = key;  // wins if that member turns out a representative
        }
        bool needs = false;
        for (uint32_t e = lo; e < hi; ++e) {
            const Pair &pr = B.pairs[B.order[e]];
            if (status[pr.r - B.b0] == ST_MEMBER || (pr.flags & F_EVAL)) continue;
            if (pair_key(pr, B.n) < win) { flight.push_back(B.order[e]); needs = true; }
        }
        if (needs || open_acc < win) { any_open = true; continue; }
        if (win != kNoBest) {
            status[q] = ST_MEMBER;
            winner_key[q] = win; iden_of[k] = win_iden; strand_of[k] = (uint8_t)(win >> 63);
        } else {
            status[q] = ST_REP;
        }
    }
    if (!any_open) return WALK_DONE;
    while (t_first < B.n_members && status[B.members[t_first] - B.b0] != ST_OPEN) ++t_first;
    return WALK_OPEN;
}

// what the one-by-one pass of the sequential rule would have examined (pgx_cluster_stats)
struct PairCounts { uint64_t filter_pairs = 0, aligned_pairs = 0, aligned_rep_len = 0, dp_cells = 0; };
inline void count_examined(const Pair &p, uint32_t len_q, uint32_t len_r, PairCounts &c) {
    c.filter_pairs++;
    if (pair_is_aligned(p)) {
        c.aligned_pairs++;
        c.aligned_rep_len += len_r;
        c.dp_cells += (uint64_t)len_q * (uint64_t)(p.band_right - p.band_left + 1);
    }
}

// A decided block: the in-block candidates the one-by-one pass examines -- the representatives among a member's
// candidates, in key order up to and including its winner (all of them for a new representative).
inline void finish_block(const Block &B, const uint8_t *status, const unsigned long long *winner_key, const uint32_t *len,
                         PairCounts &c) {
    for (uint32_t t = 0; t < B.n_members; ++t) {
        const uint32_t k = B.members[t], q = k - B.b0;
        const unsigned long long win = status[q] == ST_MEMBER ? winner_key[q] : kNoBest;
        for (uint32_t e = B.bucket[t]; e < B.bucket[t + 1]; ++e) {
            const Pair &pr = B.pairs[B.order[e]];
            if (status[pr.r - B.b0] != ST_REP) continue;
            if (pair_key(pr, B.n) > win) continue;
            count_examined(pr, len[k], len[pr.r], c);
        }
    }
}

// The pair records a window's close published (q = member of the window or its reverse complement, r = sorted sequence
// index of a representative; len[] = lengths by sorted sequence index), after the members' states and winners are final.
// Counts the candidates the one-by-one pass examines -- in key order up to and including the winner, all of them for a
// member that found none -- and notes the winner's identity. Returns false when some pair passed the diagonal test with
// a band the aligner cannot take.
inline bool finish_window_pairs(const Pair *pairs, uint32_t n_pairs, uint32_t b0, uint32_t n, const uint8_t *status,
                                const unsigned long long *winner_key, const uint32_t *len, int32_t *iden_of,
                                PairCounts &c) {
    bool fits = true;
    for (uint32_t i = 0; i < n_pairs; ++i) {
        const Pair &p = pairs[i];
        const uint32_t k = real_seq(p.q, n), q = k - b0;
        if (pair_band_too_wide(p)) { fits = false; continue; }
        const unsigned long long key = pair_key(p, n);
        if (status[q] == ST_REP || status[q] == ST_NONE || key <= winner_key[q]) {
            count_examined(p, len[k], len[p.r], c);
            if ((p.flags & F_ACCEPT) && status[q] == ST_MEMBER && key == winner_key[q]) iden_of[k] = p.iden;
        }
    }
    return fits;
}

}  // namespace pgxc
