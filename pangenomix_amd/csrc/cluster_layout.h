// Layout of the sorted list of a clustering call from its length histogram (host side, plain C++: no HIP, so that a
// stand-alone program can exercise it; tests/cluster_layout_check.cpp).
//
// The sorted list (stable, descending length) is one RUN of equal lengths per histogram bucket: run r holds the
// hist[max_len - r] sequences of max_len - r letters. Per run: its first sorted position, the residue offset and the
// offset in 5-bit packed words (six residues per word) of its first sequence -- prefix sums over the buckets, n_runs + 1
// = max_len + 2 entries each, the last = the totals. Inside a run the offsets advance by the length.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace pgxc {

// Fills the three tables (max_len + 2 entries each) and returns the packed words of all sequences in 64 bits: run_pk is
// only meaningful when that fits 32 bits, which is the caller's to check.
inline uint64_t build_run_tables(const uint32_t *hist, uint32_t max_len, uint64_t *run_off, uint32_t *run_pos,
                                 uint32_t *run_pk) {
    const uint32_t n_runs = max_len + 1;
    uint64_t pos = 0, off = 0, pk = 0;
    for (uint32_t r = 0; r < n_runs; ++r) {
        run_pos[r] = (uint32_t)pos; run_off[r] = off; run_pk[r] = (uint32_t)pk;
        const uint64_t L = max_len - r, c = hist[L];
        pos += c; off += c * L; pk += c * ((L + 5) / 6);
    }
    run_pos[n_runs] = (uint32_t)pos; run_off[n_runs] = off; run_pk[n_runs] = (uint32_t)pk;
    return pk;
}

// len[k] and off[k] for sorted positions k in [b, e), b < e <= nv, of a list of n sequences followed (nv = 2 n: both
// strands) by a second copy of the same lengths whose residues lie behind the first copy's.
inline void expand_runs(const uint64_t *run_off, const uint32_t *run_pos, uint32_t max_len, uint32_t n, size_t b,
                        size_t e, uint32_t *len, uint64_t *off) {
    if (b >= e) return;
    const uint32_t n_runs = max_len + 1;
    size_t kk = b >= n ? b - n : b;
    uint32_t r = (uint32_t)(std::upper_bound(run_pos, run_pos + n_runs + 1, (uint32_t)kk) - run_pos) - 1;
    for (size_t k = b; k < e; ++k, ++kk) {
        if (kk == n) { kk = 0; r = 0; }
        while (run_pos[r + 1] <= kk) ++r;   // (skips empty runs)
        const uint32_t L = max_len - r;
        len[k] = L;
        off[k] = (k >= n ? run_off[n_runs] : 0) + run_off[r] + (uint64_t)(kk - run_pos[r]) * L;
    }
}

// first sorted position whose sequence has at most `cap` words of `word_len` letters: behind the runs of longer ones
inline uint32_t first_with_words_le(const uint32_t *run_pos, uint32_t max_len, uint32_t cap, int word_len) {
    const uint64_t fits = (uint64_t)cap + (uint64_t)word_len - 1;   // the longest such sequence
    return max_len > fits ? run_pos[max_len - (uint32_t)fits] : 0u;
}

}  // namespace pgxc
