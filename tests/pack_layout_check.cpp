// Stand-alone check of pangenomix_amd/csrc/pgx_pack.h (tests/test_pack_layout_host.py builds it with
// -fsanitize=address,undefined and runs it): the offsets PackLayout::add hands out against WsLayout::take as the library
// had it before the two shared one rule, restated here -- on parts of 0, 1, 255, 256, 257 bytes and of more than 2^32, and
// on sequences with zero-byte parts first, last and side by side.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../pangenomix_amd/csrc/pgx_pack.h"

static int failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { ++failures; std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } \
    } while (0)

struct TakeLayout {      // WsLayout::take, word for word
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t o = off;
        off += (bytes + 255) & ~(size_t)255;
        return o;
    }
};

static size_t rounded(size_t bytes) { return (bytes + 255) / 256 * 256; }

static void one_case(const std::vector<size_t> &sizes) {
    PackLayout lay;
    TakeLayout want;
    CHECK(lay.total() == 0);
    std::vector<PackPart> parts;
    for (size_t bytes : sizes) {
        const PackPart part = lay.add(bytes);
        CHECK(part.off == want.take(bytes));
        CHECK(part.bytes == bytes);
        CHECK(part.off % 256 == 0);
        CHECK(lay.total() == want.off);
        CHECK(lay.total() == part.off + rounded(bytes));      // the last offset plus the rounded size
        parts.push_back(part);
    }
    // no two parts overlap: each ends before the next one of them starts (a zero-byte part holds no byte at all)
    for (size_t i = 0; i < parts.size(); ++i)
        for (size_t j = i + 1; j < parts.size(); ++j) {
            CHECK(parts[i].off <= parts[j].off);
            CHECK(parts[i].off + parts[i].bytes <= parts[j].off);
            CHECK(parts[j].off + parts[j].bytes <= lay.total());
        }
}

int main() {
    static_assert(sizeof(size_t) == 8, "sizes above 2^32 need a 64-bit size_t");
    const size_t huge = ((size_t)1 << 32) + 5;
    const std::vector<size_t> edge = {0, 1, 255, 256, 257, huge};
    one_case({});
    for (size_t a : edge) {
        one_case({a});
        for (size_t b : edge) {
            one_case({a, b});
            for (size_t c : edge) one_case({a, b, c});
        }
    }
    one_case({0, 0, 7, 0});                   // leading, consecutive and trailing zero-byte parts
    one_case({0, 0, 0});
    one_case({300, 0, 0, 1, 0, 0});
    one_case({0, huge, 0, 0, huge, 257, 0});
    std::mt19937_64 rng(11);
    for (int round = 0; round < 300; ++round) {
        std::vector<size_t> sizes(1 + rng() % 12);
        for (size_t &bytes : sizes) {
            const unsigned kind = (unsigned)(rng() % 4);
            bytes = kind == 0 ? 0 : kind == 1 ? edge[rng() % edge.size()] : kind == 2 ? rng() % 2000 : rng() % ((size_t)1 << 36);
        }
        one_case(sizes);
    }
    if (failures) { std::fprintf(stderr, "%d failure(s)\n", failures); return 1; }
    std::puts("pack_layout: ok");
    return 0;
}
