// Stand-alone check of pangenomix_amd/csrc/cluster_layout.h (tests/test_cluster_layout_host.py builds it with
// -fsanitize=address,undefined and runs it): the run tables and their expansion against a sort done the plain way,
// on histograms with empty buckets, one bucket, one sequence, both strands, and shares that start and end anywhere.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../pangenomix_amd/csrc/cluster_layout.h"

static int failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { ++failures; std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } \
    } while (0)

static void one_case(const std::vector<uint32_t> &lens, bool both, unsigned shares, int word_len) {
    uint32_t max_len = 0;
    for (uint32_t L : lens) max_len = std::max(max_len, L);
    std::vector<uint32_t> hist((size_t)max_len + 1, 0);
    for (uint32_t L : lens) hist[L]++;
    const uint32_t n = (uint32_t)lens.size(), nv = both ? 2 * n : n, n_runs = max_len + 1;
    // exactly as many entries as the functions may touch: the sanitizer sees anything beyond
    std::vector<uint64_t> run_off((size_t)n_runs + 1);
    std::vector<uint32_t> run_pos((size_t)n_runs + 1), run_pk((size_t)n_runs + 1);
    const uint64_t pk = pgxc::build_run_tables(hist.data(), max_len, run_off.data(), run_pos.data(), run_pk.data());
    std::vector<uint32_t> sorted(lens);
    std::stable_sort(sorted.begin(), sorted.end(), [](uint32_t a, uint32_t b) { return a > b; });
    std::vector<uint32_t> want_len(nv);
    std::vector<uint64_t> want_off((size_t)nv + 1, 0);
    uint64_t want_pk = 0;
    for (uint32_t k = 0; k < nv; ++k) {
        want_len[k] = sorted[k % n];
        want_off[k + 1] = want_off[k] + want_len[k];
        if (k < n) want_pk += (want_len[k] + 5) / 6;
    }
    CHECK(pk == want_pk);
    CHECK(run_pos[n_runs] == n && run_off[n_runs] == want_off[n]);
    std::vector<uint32_t> len(nv, 0xFFFFFFFFu);
    std::vector<uint64_t> off(nv, ~0ull);
    const size_t per = (nv + shares - 1) / shares;
    for (unsigned t = 0; t < shares; ++t)
        pgxc::expand_runs(run_off.data(), run_pos.data(), max_len, n, std::min<size_t>(nv, t * per),
                          std::min<size_t>(nv, (t + 1) * per), len.data(), off.data());
    for (uint32_t k = 0; k < nv; ++k) {
        CHECK(len[k] == want_len[k]);
        CHECK(off[k] == want_off[k]);
        if (failures > 20) return;
    }
    for (uint32_t cap : {1u, 7u, 512u, 1023u, 2048u, 8192u, 32768u}) {
        uint32_t want = 0;
        while (want < n && sorted[want] - word_len + 1 > cap) ++want;
        CHECK(pgxc::first_with_words_le(run_pos.data(), max_len, cap, word_len) == want);
    }
}

int main() {
    std::mt19937 rng(7);
    one_case({11}, false, 1, 5);
    one_case({11}, true, 3, 5);
    one_case({40, 40, 40, 40}, true, 3, 5);
    one_case({5, 900, 5, 5, 900, 33}, false, 4, 2);
    for (int round = 0; round < 200; ++round) {
        const uint32_t n = 1 + rng() % 700, span = 1 + rng() % (round % 4 == 0 ? 40000 : 60), lo = 4 + rng() % 50;
        std::vector<uint32_t> lens(n);
        for (uint32_t &L : lens) L = lo + rng() % span;
        one_case(lens, round % 2 == 1, 1 + rng() % 9, 2 + (int)(rng() % 4));
    }
    if (failures) { std::fprintf(stderr, "%d failure(s)\n", failures); return 1; }
    std::puts("cluster_layout: ok");
    return 0;
}
