// Device helpers for byte strings kept in a blob with offsets: a string's span clamped into the blob and its 16-byte chunks
// read without touching a byte outside it (dict.hip, prox.hip, pattern.hip, near.hip), the order-free 64-bit hash a group of
// DM_GROUP lanes computes of a string (dict.hip and prox.hip; dict.hip's header comment has the scheme), and the 64-bit mix
// under it, which annot.hip takes for its hashes of token lists.
#pragma once
#include "pgx_internal.h"

namespace string_hash {

constexpr uint32_t DM_GROUP = 16;                          // lanes per string
constexpr uint32_t DM_CHUNK = 16;                          // bytes per lane and step

typedef unsigned long long u64;

struct Chunk {
    u64 lo, hi;
};

// The n (1..16) bytes at blob[pos .. pos + n), zero-padded to 16. total = the blob's bytes; pos + n <= total.
__device__ __forceinline__ Chunk load_chunk(const uint8_t *__restrict__ blob, u64 total, u64 pos, uint32_t n) {
    const uint8_t *p = blob + pos;
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u);
    Chunk c;
    // the aligned word that holds p starts mis bytes before it; a second one is needed when the bytes run past its end
    const bool two = mis + n > 16u;
    if (pos >= mis && pos - mis + (two ? 32u : 16u) <= total) {
        const uint4 *w = reinterpret_cast<const uint4 *>(p - mis);
        const uint4 a = w[0];
        u64 q0 = ((u64)a.y << 32) | a.x, q1 = ((u64)a.w << 32) | a.z, q2 = 0, q3 = 0;
        if (two) {
            const uint4 b = w[1];
            q2 = ((u64)b.y << 32) | b.x;
            q3 = ((u64)b.w << 32) | b.z;
        }
        uint32_t s = mis * 8u;
        if (s >= 64u) { q0 = q1; q1 = q2; q2 = q3; s -= 64u; }
        c.lo = s ? (q0 >> s) | (q1 << (64u - s)) : q0;
        c.hi = s ? (q1 >> s) | (q2 << (64u - s)) : q1;
        if (n < 16u) {                                     // bytes n.. are not the string's
            if (n <= 8u) { c.hi = 0; c.lo = n == 8u ? c.lo : c.lo & ((1ull << (n * 8u)) - 1ull); }
            else c.hi &= (1ull << ((n - 8u) * 8u)) - 1ull;
        }
    } else {
        c.lo = c.hi = 0;
        for (uint32_t j = 0; j < n; ++j) {
            const u64 b = p[j];
            if (j < 8u) c.lo |= b << (j * 8u);
            else c.hi |= b << ((j - 8u) * 8u);
        }
    }
    return c;
}

__device__ __forceinline__ u64 fmix(u64 h) {
    h ^= h >> 33; h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33; h *= 0xC4CEB9FE1A85EC53ull;
    h ^= h >> 33;
    return h;
}

__device__ __forceinline__ u64 mix_chunk(const Chunk &c, u64 number) {
    const u64 x = (c.lo ^ (0x9E3779B97F4A7C15ull * (2ull * number + 1ull))) * 0xBF58476D1CE4E5B9ull;
    const u64 y = (c.hi + 0xC2B2AE3D27D4EB4Full * (number + 1ull)) * 0x94D049BB133111EBull;
    return fmix(x ^ ((y << 31) | (y >> 33)));
}

// [begin, begin + len) of string i, clamped into the blob whatever the offsets hold (the host entries have checked them;
// a device caller's are trusted for the result, not for memory safety).
__device__ __forceinline__ void string_span(const u64 *__restrict__ offsets, uint32_t i, u64 total, u64 &begin, u64 &len) {
    u64 b = offsets[i], e = offsets[i + 1];
    b = b < total ? b : total;
    e = e < total ? e : total;
    begin = b;
    len = e > b ? e - b : 0;
}

// The hash of a string, on every lane of the group that owns it (sub = the lane's place in the group). first = the lane's
// chunk of the first step (zero beyond the string), kept for the compare.
__device__ __forceinline__ u64 group_hash(const uint8_t *__restrict__ blob, u64 total, u64 begin, u64 len, uint32_t sub,
                                          uint32_t flags, Chunk &first) {
    u64 sum = 0;
    first.lo = first.hi = 0;
    const u64 n_chunks = (len + DM_CHUNK - 1) / DM_CHUNK;
    for (u64 c = sub; c < n_chunks; c += DM_GROUP) {
        const u64 left = len - c * DM_CHUNK;
        const Chunk ch = load_chunk(blob, total, begin + c * DM_CHUNK, left < DM_CHUNK ? (uint32_t)left : DM_CHUNK);
        if (c == sub) first = ch;
        sum += mix_chunk(ch, c);
    }
    // (every lane of the wave gets here: the trip counts differ, the shuffles come after the loop)
    for (uint32_t d = DM_GROUP / 2; d >= 1; d >>= 1) {
        const uint32_t lo = __shfl_xor((int)(uint32_t)sum, (int)d, (int)DM_GROUP);
        const uint32_t hi = __shfl_xor((int)(uint32_t)(sum >> 32), (int)d, (int)DM_GROUP);
        sum += ((u64)hi << 32) | lo;
    }
    const u64 h = fmix(sum + len * 0xD6E8FEB86659FD93ull + 0x2545F4914F6CDD1Dull);
    return (flags & PGX_DICT_NARROW_HASH) ? (h & 7ull) : h;
}

}  // namespace string_hash
