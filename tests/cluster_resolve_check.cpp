// Stand-alone check of pangenomix_amd/csrc/cluster_resolve.h (tests/test_cluster_resolve_host.py builds it with
// -fsanitize=address,undefined and runs it): the in-order walk of a block against the sequential rule written the naive
// way, with this program playing the device; window formation against a restatement; the threshold tables against the
// same expressions in double; the counting passes against direct counts. Every buffer has exactly the entries the
// functions may touch, so the sanitizer sees anything beyond.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../pangenomix_amd/csrc/cluster_resolve.h"

using namespace pgxc;
typedef unsigned long long u64;

static int failures = 0;
static const char *g_case = "";
#define CHECK(cond)                                                                                   \
    do {                                                                                              \
        if (!(cond)) { ++failures; std::fprintf(stderr, "%s: line %d: %s\n", g_case, __LINE__, #cond); } \
    } while (0)

// ---- the block walk ---------------------------------------------------------------------------------------------
struct TruePair { uint32_t q, r, minc; uint32_t flags; int32_t iden; bool evaluated; };   // flags: what the device would find
struct BlockCase {
    const char *name;
    uint32_t b0, n;
    std::vector<uint32_t> members;   // ascending sorted sequence indices, >= b0
    std::vector<TruePair> pairs;     // q = a member or its reverse complement (+ n), r = an earlier member
    bool expect_band = false;
};

static u64 naive_key(const TruePair &p, uint32_t n) { return ((u64)(p.q >= n ? 1 : 0) << 63) | ((u64)p.minc << 32) | (u64)p.r; }

static void run_block(BlockCase bc) {
    g_case = bc.name;
    const uint32_t nm = (uint32_t)bc.members.size(), np = (uint32_t)bc.pairs.size(), b0 = bc.b0, n = bc.n;
    const uint32_t last = bc.members.back(), nw = last - b0 + 1;
    // the sequential rule, the naive way: members in order; the winner is the smallest key among the member's accepted
    // pairs whose r has been decided a representative; without one the member is a representative
    std::vector<uint8_t> want_status(nw, ST_MEMBER), want_strand((size_t)last + 1, 7);
    std::vector<u64> want_key(nw, 0);
    std::vector<int32_t> want_iden((size_t)last + 1, -7);
    for (uint32_t k : bc.members) want_status[k - b0] = ST_OPEN;
    if (!bc.expect_band)
        for (uint32_t k : bc.members) {
            u64 best = kNoBest; int32_t iden = 0;
            for (const TruePair &p : bc.pairs) {
                if ((p.q >= n ? p.q - n : p.q) != k || !(p.flags & F_ACCEPT)) continue;
                if (want_status[p.r - b0] != ST_REP) continue;
                if (naive_key(p, n) < best) { best = naive_key(p, n); iden = p.iden; }
            }
            if (best == kNoBest) { want_status[k - b0] = ST_REP; continue; }
            want_status[k - b0] = ST_MEMBER; want_key[k - b0] = best; want_iden[k] = iden; want_strand[k] = (uint8_t)(best >> 63);
        }
    // what the host sees: a record carries the device's findings once it has been evaluated
    std::vector<Pair> vis(np);
    auto publish = [&](uint32_t i) {
        const TruePair &p = bc.pairs[i];
        vis[i] = Pair{p.q, p.r, 1u, p.minc, 0, -3, 0, 3, p.evaluated ? p.iden : 0, p.evaluated ? (p.flags | F_EVAL) : 0u};
    };
    for (uint32_t i = 0; i < np; ++i) publish(i);
    std::vector<uint32_t> rank_of(nw, 0xFFFFFFFFu), bucket((size_t)nm + 1), fill(nm), order(np);
    bucket_block_pairs(bc.members.data(), nm, vis.data(), np, b0, n, rank_of.data(), bucket.data(), fill.data(), order.data());
    CHECK(bucket[0] == 0 && bucket[nm] == np);
    {   // a permutation, every pair in its query's bucket, in record order inside a bucket
        std::vector<uint8_t> seen(np, 0);
        for (uint32_t t = 0; t < nm; ++t)
            for (uint32_t e = bucket[t]; e < bucket[t + 1]; ++e) {
                CHECK(order[e] < np);
                if (order[e] >= np) return;
                CHECK(!seen[order[e]]); seen[order[e]] = 1;
                CHECK(real_seq(vis[order[e]].q, n) == bc.members[t]);
                CHECK(e == bucket[t] || order[e - 1] < order[e]);
            }
        for (uint32_t i = 0; i < np; ++i) CHECK(seen[i]);
    }
    std::vector<uint8_t> status(nw, ST_MEMBER), strand((size_t)last + 1, 7);
    std::vector<u64> key(nw, 0);
    std::vector<int32_t> iden((size_t)last + 1, -7);
    for (uint32_t k : bc.members) status[k - b0] = ST_OPEN;
    const Block B{bc.members.data(), nm, vis.data(), np, b0, n, bucket.data(), order.data()};
    std::vector<uint32_t> flight;
    uint32_t t_first = 0, passes = 0;
    WalkResult w;
    for (;;) {
        w = walk_block(B, t_first, status.data(), key.data(), iden.data(), strand.data(), flight);
        ++passes;
        CHECK(passes <= nm);
        if (w != WALK_OPEN || passes > nm) break;
        bool open_left = false;
        for (uint32_t k : bc.members) open_left |= status[k - b0] == ST_OPEN;
        CHECK(open_left);
        CHECK(!flight.empty());   // a pass that leaves a member open asks for something
        if (flight.empty()) break;
        CHECK(t_first < nm && status[bc.members[t_first] - b0] == ST_OPEN);
        std::set<uint32_t> once(flight.begin(), flight.end());
        CHECK(once.size() == flight.size());
        for (uint32_t i : flight) {
            CHECK(i < np);
            if (i >= np) return;
            CHECK(!(vis[i].flags & F_EVAL));   // ... that has not been evaluated
        }
        for (uint32_t i : flight) { bc.pairs[i].evaluated = true; publish(i); }
    }
    if (bc.expect_band) { CHECK(w == WALK_BAND); return; }
    CHECK(w == WALK_DONE);
    CHECK(status == want_status);
    for (uint32_t k : bc.members)
        if (want_status[k - b0] == ST_MEMBER) CHECK(key[k - b0] == want_key[k - b0]);
    CHECK(iden == want_iden);
    CHECK(strand == want_strand);

    // the counting pass against a direct count: the representatives among a member's candidates up to its winner
    std::vector<uint32_t> len((size_t)last + 1);
    for (uint32_t k = 0; k <= last; ++k) len[k] = 30 + (k * 7) % 50;
    PairCounts got, want;
    finish_block(B, status.data(), key.data(), len.data(), got);
    for (uint32_t i = 0; i < np; ++i) {
        const Pair &p = vis[i];
        const uint32_t k = real_seq(p.q, n);
        if (status[p.r - b0] != ST_REP) continue;
        if (status[k - b0] == ST_MEMBER && pair_key(p, n) > key[k - b0]) continue;
        want.filter_pairs++;
        if ((p.flags & F_DIAG_PASS) && (p.flags & F_BAND_OK)) {
            want.aligned_pairs++; want.aligned_rep_len += len[p.r];
            want.dp_cells += (uint64_t)len[k] * (uint64_t)(p.band_right - p.band_left + 1);
        }
    }
    CHECK(got.filter_pairs == want.filter_pairs && got.aligned_pairs == want.aligned_pairs);
    CHECK(got.aligned_rep_len == want.aligned_rep_len && got.dp_cells == want.dp_cells);
}

static const uint32_t kAcc = F_DIAG_PASS | F_BAND_OK | F_ALIGNED | F_ACCEPT, kRej = F_DIAG_PASS | F_BAND_OK | F_ALIGNED;

static void named_blocks() {
    run_block({"one member, no pairs", 100, 1000, {100}, {}});
    run_block({"two members, one accepted pair", 100, 1000, {103, 110}, {{110, 103, 5, kAcc, 42, true}}});
    run_block({"two members, one accepted pair, not evaluated", 100, 1000, {103, 110}, {{110, 103, 5, kAcc, 42, false}}});
    run_block({"two members, one rejected pair", 0, 1000, {0, 1}, {{1, 0, 5, kRej, 3, false}}});
    for (uint32_t k : {2u, 3u, 8u, 9u, 33u}) {   // each member accepted only by the one before, nothing evaluated up front:
        BlockCase c{"dependency chain", 50, 1000, {}, {}};   // representatives and members alternate (the walk lists every pair
        for (uint32_t i = 0; i < k; ++i) {                   // in its first pass, so two passes decide the chain whatever k)
            c.members.push_back(50 + 2 * i);
            if (i) c.pairs.push_back({50 + 2 * i, 50 + 2 * (i - 1), 9, kAcc, (int32_t)i, false});
        }
        run_block(c);
    }
    {   // ... with every other pair evaluated up front
        BlockCase c{"dependency chain, every other pair evaluated", 50, 1000, {}, {}};
        for (uint32_t i = 0; i < 12; ++i) {
            c.members.push_back(50 + i);
            if (i) c.pairs.push_back({50 + i, 50 + i - 1, 9, kAcc, (int32_t)i, i % 2 == 0});
        }
        run_block(c);
    }
    // 12 joins 10; 13's smaller key is against 12 (a member: ignored), so 13 joins 11
    run_block({"accepted pair whose r ends as a member", 10, 1000, {10, 11, 12, 13},
               {{12, 10, 4, kAcc, 30, true}, {13, 12, 1, kAcc, 31, false}, {13, 11, 8, kAcc, 32, false}}});
    run_block({"equal minc, tie broken by r", 10, 1000, {10, 11, 12},
               {{12, 11, 6, kAcc, 21, false}, {12, 10, 6, kAcc, 20, true}}});
    // the reverse complement of 12 (q = 12 + n) has the smaller code, the forward strand still goes first; 13 is placed by
    // its reverse strand alone
    run_block({"reverse-strand query", 10, 40, {10, 11, 12, 13},
               {{12 + 40, 10, 1, kAcc, 20, false}, {12, 11, 9, kAcc, 21, true}, {13 + 40, 11, 2, kAcc, 22, false}}});
    run_block({"evaluated too-big pair that passed the diagonal test", 10, 1000, {10, 11},
               {{11, 10, 3, F_TOO_BIG | F_DIAG_PASS, 0, true}}, true});
    run_block({"too-big pair found by a follow-up round", 10, 1000, {10, 11, 12},
               {{12, 10, 3, F_TOO_BIG | F_DIAG_PASS, 0, false}, {12, 11, 5, kAcc, 9, true}}, true});
    run_block({"too-big pair that failed the diagonal test is no error", 10, 1000, {10, 11}, {{11, 10, 3, F_TOO_BIG, 0, true}}});
}

static void random_blocks(std::mt19937 &rng) {
    for (int round = 0; round < 400; ++round) {
        const std::string name = "random block " + std::to_string(round);
        BlockCase c{name.c_str(), (uint32_t)(rng() % 1000), 0, {}, {}};
        const uint32_t nm = 1 + rng() % 64, want_pairs = rng() % 401;
        const bool both = round % 3 == 0;
        uint32_t k = c.b0 + rng() % 3;
        for (uint32_t i = 0; i < nm; ++i) { c.members.push_back(k); k += 1 + rng() % 3; }
        c.n = both ? k + rng() % 5 : 100000;   // both strands: n just above the last member
        const uint32_t accept_pct = (uint32_t)(rng() % 101), eval_pct = round % 5 == 0 ? 0 : (round % 5 == 1 ? 100 : (uint32_t)(rng() % 101));
        std::set<std::pair<uint32_t, uint32_t>> used;
        for (uint32_t i = 0; i < want_pairs && nm > 1; ++i) {
            const uint32_t tq = 1 + rng() % (nm - 1), tr = rng() % tq;
            const uint32_t q = c.members[tq] + (both && rng() % 2 ? c.n : 0u), r = c.members[tr];
            if (!used.insert({q, r}).second) continue;
            const bool acc = rng() % 100 < accept_pct;
            const uint32_t kind = rng() % 4;   // rejected pairs: after the alignment, by the band test, by the diagonal test
            const uint32_t flags = acc ? kAcc : (kind == 0 ? kRej : (kind == 1 ? F_DIAG_PASS : (kind == 2 ? 0u : F_TOO_BIG)));
            c.pairs.push_back({q, r, (uint32_t)(rng() % 6), flags, (int32_t)(rng() % 500), rng() % 100 < eval_pct});
        }
        run_block(c);
        if (failures > 20) return;
    }
}

// ---- the window's published pairs ---------------------------------------------------------------------------------
static void window_pairs(std::mt19937 &rng) {
    g_case = "finish_window_pairs";
    for (int round = 0; round < 100; ++round) {
        const bool both = round % 2 == 1, with_wide = round % 10 == 9;
        const uint32_t b0 = 200 + rng() % 50, nb = 1 + rng() % 40, n = both ? b0 + nb + rng() % 4 : 5000, np = rng() % 300;
        std::vector<uint8_t> status(nb);
        std::vector<u64> key(nb, 0);
        for (uint32_t q = 0; q < nb; ++q) {
            const uint32_t s = rng() % 4;
            status[q] = s == 0 ? ST_REP : (s == 1 ? ST_NONE : ST_MEMBER);
            key[q] = ((u64)(both && rng() % 2) << 63) | ((u64)(rng() % 4) << 32) | (rng() % b0);
        }
        std::vector<uint32_t> len((size_t)b0 + nb);
        for (uint32_t &L : len) L = 20 + rng() % 300;
        std::vector<Pair> pairs(np);
        for (Pair &p : pairs) {
            const uint32_t q = rng() % nb;
            p = Pair{b0 + q + (both && rng() % 2 ? n : 0u), (uint32_t)(rng() % b0), 1u, (uint32_t)(rng() % 4), 0, -(int32_t)(rng() % 9),
                     0, (int32_t)(rng() % 9), (int32_t)(rng() % 200), 0u};
            const uint32_t kind = rng() % 4;
            p.flags = F_EVAL | (kind == 0 ? kAcc : (kind == 1 ? kRej : (kind == 2 ? F_DIAG_PASS : 0u)));
            if (rng() % 6 == 0 && status[q] == ST_MEMBER) {   // the winner's own record
                p.q = b0 + q + ((key[q] >> 63) ? n : 0u); p.minc = (uint32_t)(key[q] >> 32) & 0x7FFFFFFFu; p.r = (uint32_t)key[q];
                p.flags = F_EVAL | kAcc;
            }
        }
        if (with_wide && np) pairs[rng() % np].flags = F_EVAL | F_TOO_BIG | F_DIAG_PASS;
        std::vector<int32_t> iden((size_t)b0 + nb, -1), want_iden(iden);
        PairCounts got, want;
        bool want_fits = true;
        for (const Pair &p : pairs) {
            const uint32_t k = p.q >= n ? p.q - n : p.q, q = k - b0;
            if ((p.flags & F_TOO_BIG) && (p.flags & F_DIAG_PASS)) { want_fits = false; continue; }
            const u64 pk = ((u64)(p.q >= n) << 63) | ((u64)p.minc << 32) | p.r;
            if (status[q] == ST_MEMBER && pk > key[q]) continue;
            want.filter_pairs++;
            if ((p.flags & F_DIAG_PASS) && (p.flags & F_BAND_OK)) {
                want.aligned_pairs++; want.aligned_rep_len += len[p.r];
                want.dp_cells += (uint64_t)len[k] * (uint64_t)(p.band_right - p.band_left + 1);
            }
            if (status[q] == ST_MEMBER && pk == key[q] && (p.flags & F_ACCEPT)) want_iden[k] = p.iden;
        }
        const bool fits = finish_window_pairs(pairs.data(), np, b0, n, status.data(), key.data(), len.data(), iden.data(), got);
        CHECK(fits == want_fits);
        CHECK(got.filter_pairs == want.filter_pairs && got.aligned_pairs == want.aligned_pairs);
        CHECK(got.aligned_rep_len == want.aligned_rep_len && got.dp_cells == want.dp_cells);
        CHECK(iden == want_iden);
    }
}

// ---- window formation ---------------------------------------------------------------------------------------------
// restated: fill chunks one sequence at a time; a sequence that does not fit the chunk volume opens the next chunk
// unless the chunk is empty; the window ends at the limit, at window_cap members, or when a 33rd chunk would open
static void one_window(const char *name, const std::vector<uint32_t> &len_all, uint32_t b0, uint32_t limit, uint32_t window_cap,
                       bool chunking, uint64_t chunk_words) {
    g_case = name;
    const std::vector<uint32_t> len(len_all.begin(), len_all.begin() + limit);   // nothing at or beyond the limit is read
    std::vector<std::vector<uint32_t>> chunks(1);
    uint64_t vol = 0;
    uint32_t nb = 0;
    for (uint32_t k = b0; k < limit && nb < window_cap; ++k) {
        if (chunking && !chunks.back().empty() && vol + len[k] > chunk_words) {
            if (chunks.size() == kMaxChunks) break;
            chunks.emplace_back(); vol = 0;
        }
        chunks.back().push_back(k); vol += len[k]; ++nb;
    }
    Chunks C;
    for (uint32_t &b : C.begin) b = 0xDEADBEEFu;
    const uint32_t got = form_window(len.data(), b0, limit, window_cap, chunking, chunk_words, C);
    CHECK(got == nb);
    CHECK(got <= window_cap && b0 + got <= limit);
    CHECK(C.n >= 1 && C.n <= kMaxChunks && C.n == chunks.size());
    if (C.n < 1 || C.n > kMaxChunks) return;
    CHECK(C.begin[0] == 0 && C.begin[C.n] == got);
    uint32_t at = 0;
    for (uint32_t c = 0; c < C.n; ++c) {
        CHECK(C.begin[c] <= C.begin[c + 1]);
        CHECK(c < chunks.size() && C.begin[c] == at);
        if (c < chunks.size()) at += (uint32_t)chunks[c].size();
        uint64_t v = 0;
        for (uint32_t q = C.begin[c]; q < C.begin[c + 1] && q < got; ++q) v += len[b0 + q];
        if (chunking) CHECK(v <= chunk_words || C.begin[c + 1] - C.begin[c] == 1);
        if (got) CHECK(C.begin[c + 1] > C.begin[c]);   // no empty chunk in a window that has members
    }
    if (!chunking) CHECK(C.n == 1);
}

static void windows(std::mt19937 &rng) {
    const std::vector<uint32_t> tens(200, 10);
    one_window("chunks closed exactly at chunk_words", tens, 0, 200, 64, true, 50);       // five per chunk: the sixth would exceed it
    one_window("kMaxChunks reached before window_cap", tens, 0, 200, 200, true, 20);      // two per chunk: 64 members, cap 200
    one_window("window_cap reached first", tens, 3, 200, 7, true, 50);
    one_window("a limit inside the window", tens, 90, 97, 64, true, 50);
    one_window("limit at b0: an empty window", tens, 90, 90, 64, true, 50);
    one_window("chunking off", tens, 0, 200, 64, false, 50);
    one_window("chunk_words smaller than every sequence", tens, 0, 200, 64, true, 3);
    std::vector<uint32_t> giant = tens;
    giant[0] = 5000; giant[7] = 51; giant[8] = 50;
    one_window("a single sequence larger than chunk_words, first", giant, 0, 200, 64, true, 50);
    one_window("a single sequence larger than chunk_words, inside", giant, 2, 200, 64, true, 50);
    for (int round = 0; round < 300; ++round) {
        std::vector<uint32_t> len(1 + rng() % 400);
        uint32_t L = 40 + rng() % 3000;
        for (uint32_t &x : len) { x = L; if (L > 1 && rng() % 3 == 0) L -= std::min<uint32_t>(L - 1, rng() % 40); }   // descending
        const uint32_t n = (uint32_t)len.size(), b0 = rng() % n, limit = b0 + rng() % (n - b0 + 1);
        one_window("random window", len, b0, limit, 1 + rng() % 300, round % 4 != 0, 1 + rng() % 20000);
        if (failures > 20) return;
    }
}

// ---- threshold tables ---------------------------------------------------------------------------------------------
static void thresholds() {
    g_case = "threshold tables";
    const uint32_t max_len = 700;
    for (bool nt : {false, true})
        for (double identity : {0.4, 0.8, 0.95, 0.9500001, 1.0}) {
            const int word_len = nt ? 10 : 5;
            const double aas_cutoff = nt ? 0.8 : 0.6, aan_cutoff = nt ? 0.025 : 0.23;
            std::vector<int32_t> aa1((size_t)max_len + 1, -99), aas(aa1), aan(aa1);
            threshold_tables(identity, word_len, aas_cutoff, aan_cutoff, nt, max_len, aa1.data(), aas.data(), aan.data());
            for (uint32_t L = 0; L <= max_len; ++L) {
                const double len = (double)L;
                const int w1 = (int)(identity * len), kd = nt ? 4 : 2;
                CHECK(aa1[L] == w1);
                if (identity > 0.95) {
                    CHECK(aas[L] == (int)L - kd + 1 - ((int)L - w1) * kd);
                    CHECK(aan[L] == (int)L - word_len + 1 - ((int)L - w1) * word_len);
                } else {
                    CHECK(aas[L] == (int)(aas_cutoff * len));
                    CHECK(aan[L] == (int)(aan_cutoff * len));
                }
                if (failures > 20) return;
            }
        }
}

int main() {
    std::mt19937 rng(11);
    named_blocks();
    random_blocks(rng);
    window_pairs(rng);
    windows(rng);
    thresholds();
    if (failures) { std::fprintf(stderr, "%d failure(s)\n", failures); return 1; }
    std::puts("cluster_resolve: ok");
    return 0;
}
