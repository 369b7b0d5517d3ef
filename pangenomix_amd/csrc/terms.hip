// Which of T short patterns occur in each of n short strings (reference amr.py:85-244 generate_probable_hits_from_annotations
// tests every annotation of every line against every search term of every drug with Python's `in`).
// String i is the length[i] bytes of a text at start[i] (the windows of pgx_prox_cut: they may overlap or repeat); term t is
// the bytes terms[term_off[t] .. term_off[t + 1]). Bit t & 63 of word mask[i * W + (t >> 6)], W = ceil(n_terms / 64), is set
// iff term t occurs as a contiguous substring of string i; the empty term occurs in every string. With PGX_TERM_FOLD_ASCII the
// bytes 'A'-'Z' of both sides are compared as 'a'-'z' and no other byte is changed.
//
// term_scan_kernel (one plain launch, no atomics):
//   once per workgroup, in LDS: the terms (folded if asked for), their offsets, and the non-empty terms ordered by first byte
//   with a 257-entry index into that order -- thread b counts and then lists the terms whose first byte is b, so nothing is
//   shared while the index is built; thread w < W marks the empty terms of word w.
//   A group of TS_GROUP lanes owns a string and walks it in steps of TS_STEP start positions, TS_PER_LANE to a lane. At a
//   position the lane looks up the bucket of the (folded) byte there and compares each candidate term that still fits into
//   the string byte for byte with the text -- a match that runs over the end of a step is found like any other, the step only
//   hands out where matches START. A match sets the term's bit in the lane's own W words in LDS; a term whose bit the lane
//   has already set is not compared again. At the end lane w of the group ORs word w of the group's lanes and stores it.
// Every read of the text is inside the string's window, which both entries keep inside [0, text_bytes).
#include "pgx_internal.h"

namespace {

typedef unsigned long long u64;

constexpr int TS_THREADS = 256;
constexpr uint32_t TS_GROUP = 16, TS_PER_LANE = 4;
constexpr uint32_t TS_STEP = TS_GROUP * TS_PER_LANE;       // start positions per group and step (pgx_term_scan_group_bytes)
constexpr uint32_t TS_GROUPS_PER_BLOCK = TS_THREADS / TS_GROUP;
constexpr uint32_t TS_MAX_GRID = 2048;
constexpr uint32_t TS_MAX_TERMS = PGX_TERM_MAX_TERMS, TS_MAX_BYTES = PGX_TERM_MAX_BYTES;
constexpr uint32_t TS_MAX_WORDS = TS_MAX_TERMS / 64;
constexpr uint32_t TS_MAX_N = 1u << 24;
static_assert(TS_MAX_TERMS % 64 == 0 && TS_MAX_WORDS <= TS_GROUP, "lane w of a group stores word w");
static_assert(TS_MAX_TERMS % TS_THREADS == 0 && TS_THREADS == 256, "thread b owns the bucket of byte b");
static_assert(TS_MAX_BYTES < 65536 && TS_MAX_TERMS < 65536, "offsets and term numbers are kept in 16 bits");

__device__ __forceinline__ uint8_t fold_byte(uint8_t c, bool fold) {
    return fold && (uint8_t)(c - 'A') < 26u ? (uint8_t)(c | 0x20u) : c;
}

__global__ __launch_bounds__(TS_THREADS) void term_scan_kernel(const uint8_t *__restrict__ text, u64 text_bytes,
                                                               const u64 *__restrict__ start,
                                                               const uint32_t *__restrict__ length, uint32_t n,
                                                               const uint8_t *__restrict__ terms,
                                                               const uint32_t *__restrict__ term_off, uint32_t n_terms,
                                                               uint32_t term_bytes, uint32_t flags, u64 *__restrict__ out) {
    __shared__ uint8_t s_terms[TS_MAX_BYTES];
    __shared__ uint16_t s_off[TS_MAX_TERMS + 1];
    __shared__ uint16_t s_order[TS_MAX_TERMS];
    __shared__ uint16_t s_bucket[257];
    __shared__ uint16_t s_count[TS_THREADS];
    __shared__ u64 s_empty[TS_MAX_WORDS];
    __shared__ u64 s_mask[TS_MAX_WORDS][TS_THREADS];       // word w of lane `tid`: the lane's own
    const uint32_t tid = threadIdx.x, sub = tid & (TS_GROUP - 1u), base = tid & ~(TS_GROUP - 1u);
    const bool fold = (flags & PGX_TERM_FOLD_ASCII) != 0;
    const uint32_t W = (n_terms + 63u) / 64u;

    // ---- the terms and their index, once -----------------------------------------------------------------------------
    for (uint32_t i = tid; i < term_bytes; i += TS_THREADS) s_terms[i] = fold_byte(terms[i], fold);
    for (uint32_t t = tid; t <= n_terms; t += TS_THREADS) {          // offsets clamped: never past the blob
        const uint32_t o = term_off[t];
        s_off[t] = (uint16_t)(o < term_bytes ? o : term_bytes);
    }
    __syncthreads();
    // a term whose end lies before its start is taken as empty (the host entry refuses such offsets)
    uint32_t count = 0;
    for (uint32_t t = 0; t < n_terms; ++t) {
        const uint32_t b = s_off[t], e = s_off[t + 1];
        if (e > b && s_terms[b] == tid) ++count;
    }
    s_count[tid] = (uint16_t)count;
    if (tid < TS_MAX_WORDS) {
        u64 m = 0;
        for (uint32_t j = 0; j < 64u; ++j) {
            const uint32_t t = tid * 64u + j;
            if (t < n_terms && s_off[t + 1] <= s_off[t]) m |= 1ull << j;
        }
        s_empty[tid] = m;
    }
    __syncthreads();
    if (tid == 0u) {
        uint32_t sum = 0;
        for (uint32_t b = 0; b < 256u; ++b) {
            s_bucket[b] = (uint16_t)sum;
            sum += s_count[b];
        }
        s_bucket[256] = (uint16_t)sum;
    }
    __syncthreads();
    {
        uint32_t at = s_bucket[tid];
        for (uint32_t t = 0; t < n_terms; ++t) {
            const uint32_t b = s_off[t], e = s_off[t + 1];
            if (e > b && s_terms[b] == tid) s_order[at++] = (uint16_t)t;
        }
    }
    __syncthreads();

    // ---- the strings ---------------------------------------------------------------------------------------------------
    const uint32_t n_rounds = (n + TS_GROUPS_PER_BLOCK - 1u) / TS_GROUPS_PER_BLOCK;
    // every lane takes the same rounds, so the barriers are reached by whole workgroups
    for (uint32_t round = blockIdx.x; round < n_rounds; round += gridDim.x) {
        const uint32_t i = round * TS_GROUPS_PER_BLOCK + tid / TS_GROUP;
        const bool live = i < n;
        u64 begin = 0;
        uint32_t len = 0;
        if (live) {
            begin = start[i];
            len = length[i];
            if (begin > text_bytes) begin = text_bytes;
            if ((u64)len > text_bytes - begin) len = (uint32_t)(text_bytes - begin);
        }
        for (uint32_t w = 0; w < W; ++w) s_mask[w][tid] = s_empty[w];
        const uint8_t *s = text + begin;
        for (uint32_t step = 0; step < len; step += TS_STEP) {
            for (uint32_t k = 0; k < TS_PER_LANE; ++k) {
                const uint32_t p = step + k * TS_GROUP + sub;        // (neighbouring lanes read neighbouring bytes)
                if (p >= len) break;
                const uint32_t c = fold_byte(s[p], fold);
                const uint32_t room = len - p;
                for (uint32_t q = s_bucket[c], q_end = s_bucket[c + 1]; q < q_end; ++q) {
                    const uint32_t t = s_order[q];
                    const uint32_t tb = s_off[t], tl = s_off[t + 1] - tb;
                    if (tl > room) continue;
                    const u64 bit = 1ull << (t & 63u);
                    if (s_mask[t >> 6][tid] & bit) continue;
                    uint32_t j = 1;                                  // (byte 0 chose the bucket)
                    while (j < tl && fold_byte(s[p + j], fold) == s_terms[tb + j]) ++j;
                    if (j == tl) s_mask[t >> 6][tid] |= bit;
                }
            }
        }
        __syncthreads();
        if (live && sub < W) {
            u64 m = 0;
            for (uint32_t l = 0; l < TS_GROUP; ++l) m |= s_mask[sub][base + l];
            out[(size_t)i * W + sub] = m;
        }
        __syncthreads();
    }
}

// ---- launches ------------------------------------------------------------------------------------------------------------
int term_require(pgx_ctx *ctx, u64 text_bytes, uint32_t n, uint32_t n_terms, u64 term_bytes, uint32_t flags) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(text_bytes < (1ull << 32), "text_bytes must be below 2^32");
    PGX_REQUIRE(n < TS_MAX_N, "n must be below 2^24");
    PGX_REQUIRE(n_terms <= TS_MAX_TERMS, "more than PGX_TERM_MAX_TERMS terms");
    PGX_REQUIRE(term_bytes <= TS_MAX_BYTES, "more than PGX_TERM_MAX_BYTES bytes of terms");
    PGX_REQUIRE((flags & ~PGX_TERM_FOLD_ASCII) == 0, "unknown flags");
    return PGX_OK;
}

int term_launch(pgx_ctx *ctx, const uint8_t *d_text, u64 text_bytes, const u64 *d_start, const uint32_t *d_length, uint32_t n,
                const uint8_t *d_terms, const uint32_t *d_term_off, uint32_t n_terms, uint32_t term_bytes, uint32_t flags,
                u64 *d_out, hipStream_t stream) {
    const uint32_t rounds = ceil_div_u32(n, TS_GROUPS_PER_BLOCK);
    {
        ProfScope prof(ctx, "term_scan_kernel", stream);
        term_scan_kernel<<<rounds < TS_MAX_GRID ? rounds : TS_MAX_GRID, TS_THREADS, 0, stream>>>(
            d_text, text_bytes, d_start, d_length, n, d_terms, d_term_off, n_terms, term_bytes, flags, d_out);
    }
    PGX_HIP(hipGetLastError());
    return PGX_OK;
}

int term_dev(pgx_ctx *ctx, const uint8_t *d_text, u64 text_bytes, const u64 *d_start, const uint32_t *d_length, uint32_t n,
             const uint8_t *d_terms, const uint32_t *d_term_off, uint32_t n_terms, u64 term_bytes, uint32_t flags, u64 *d_out,
             hipStream_t stream) {
    int rc = term_require(ctx, text_bytes, n, n_terms, term_bytes, flags);
    if (rc != PGX_OK) return rc;
    if (n == 0 || n_terms == 0) return PGX_OK;
    PGX_REQUIRE(d_start && d_length && d_term_off && d_out, "NULL argument");
    PGX_REQUIRE((text_bytes == 0 || d_text) && (term_bytes == 0 || d_terms), "NULL text or terms");
    PGX_REQUIRE(((uintptr_t)d_start & 7u) == 0 && ((uintptr_t)d_out & 7u) == 0, "start and out_mask must be 8-byte aligned");
    rc = term_launch(ctx, d_text, text_bytes, d_start, d_length, n, d_terms, d_term_off, n_terms, (uint32_t)term_bytes, flags,
                     d_out, stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(hipStreamSynchronize(stream));
    return PGX_OK;
}

int term_host(pgx_ctx *ctx, const uint8_t *text, u64 text_bytes, const uint64_t *start, const uint32_t *length, uint32_t n,
              const uint8_t *terms, const uint32_t *term_off, uint32_t n_terms, uint32_t flags, uint64_t *out_mask) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(n_terms <= TS_MAX_TERMS, "more than PGX_TERM_MAX_TERMS terms");
    PGX_REQUIRE(term_off, "NULL term_off");
    for (uint32_t t = 0; t < n_terms; ++t) PGX_REQUIRE(term_off[t] <= term_off[t + 1], "offsets must not decrease");
    PGX_REQUIRE(term_off[0] == 0, "offsets must start at 0");
    const uint32_t term_bytes = term_off[n_terms];
    int rc = term_require(ctx, text_bytes, n, n_terms, term_bytes, flags);
    if (rc != PGX_OK) return rc;
    PGX_REQUIRE(n == 0 || (start && length), "NULL start or length");
    for (uint32_t i = 0; i < n; ++i)
        PGX_REQUIRE(start[i] <= text_bytes && length[i] <= text_bytes - start[i], "a window leaves the text");
    if (n == 0 || n_terms == 0) return PGX_OK;
    PGX_REQUIRE(out_mask && (text_bytes == 0 || text) && (term_bytes == 0 || terms), "NULL argument");
    PGX_HIP(hipSetDevice(ctx->device_id));
    const uint32_t W = ceil_div_u32(n_terms, 64);
    DevBuf d_text(ctx, TS_SLOT_TEXT);
    DevPack in(ctx, TS_SLOT_IN), res(ctx, TS_SLOT_OUT);
    const PackPart p_start = in.in(start, n), p_len = in.in(length, n), p_off = in.in(term_off, (size_t)n_terms + 1),
                   p_terms = in.in(terms, term_bytes);
    const PackPart r_mask = res.out(out_mask, (size_t)n * W);
    PGX_HIP(d_text.alloc((size_t)text_bytes));
    PGX_HIP(in.alloc());
    PGX_HIP(res.alloc());
    if (text_bytes) {
        rc = pgx_staged_h2d(ctx, d_text.p, text, (size_t)text_bytes, ctx->stream);
        if (rc != PGX_OK) return rc;
    }
    PGX_HIP(in.upload(ctx->stream));
    rc = term_launch(ctx, d_text.as<uint8_t>(), text_bytes, (const u64 *)in.dev<uint64_t>(p_start), in.dev<uint32_t>(p_len), n,
                     in.dev<uint8_t>(p_terms), in.dev<uint32_t>(p_off), n_terms, term_bytes, flags,
                     (u64 *)res.dev<uint64_t>(r_mask), ctx->stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(res.download(ctx->stream));
    PGX_HIP(hipStreamSynchronize(ctx->stream));
    return PGX_OK;
}

}  // namespace

extern "C" {

uint32_t pgx_term_scan_group_bytes(void) { return TS_STEP; }

int pgx_term_scan(pgx_ctx *ctx, const uint8_t *text, uint64_t text_bytes, const uint64_t *start, const uint32_t *length,
                  uint32_t n, const uint8_t *terms, const uint32_t *term_off, uint32_t n_terms, uint32_t flags,
                  uint64_t *out_mask) {
    return guarded(__func__, [&] {
        return term_host(ctx, text, text_bytes, start, length, n, terms, term_off, n_terms, flags, out_mask);
    });
}

int pgx_term_scan_dev(pgx_ctx *ctx, const uint8_t *d_text, uint64_t text_bytes, const uint64_t *d_start,
                      const uint32_t *d_length, uint32_t n, const uint8_t *d_terms, const uint32_t *d_term_off,
                      uint32_t n_terms, uint64_t term_bytes, uint32_t flags, uint64_t *d_out_mask, void *stream) {
    return guarded(__func__, [&] {
        return term_dev(ctx, d_text, text_bytes, (const u64 *)d_start, d_length, n, d_terms, d_term_off, n_terms, term_bytes,
                        flags, (u64 *)d_out_mask, (hipStream_t)stream);
    });
}

}  // extern "C"
