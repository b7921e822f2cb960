// digest_kernel.inl -- k_digest, k_digest_final: Adler-32 (RFC 1950, zlib's adler32(data, value)) of byte strings that lie in
// device memory as pitched rows (h263mi_adler32_spans_on, h263mi_*_digest_yuv; ABI 7).
//
// The contract (include/h263mi.h): digest k is the Adler-32 of the rows of every span with digest == k, in table order, row
// after row, row_bytes bytes each.  With N the string's length, a0 = seed & 0xffff, b0 = seed >> 16, M = 65521:
//     A = (a0 + sum d_i) mod M,   B = (b0 + N * a0 + sum (N - i) * d_i) mod M   (i from 0),   result = B << 16 | A.
// A piece of length L with T bytes of the string behind it, a_c = sum d_j, b_c = sum (L - j) * d_j over the piece, adds a_c to A
// and b_c + a_c * T to B: pieces are independent, and integer additions combine them in any order.
//
// One wave per workgroup, no barrier.  The host cuts every span into work ITEMS of at most DIGEST_PIECE bytes (digest_table):
// a run of whole rows where the rows are shorter than that (at most DIGEST_MAX_ROWS of them), else a piece of one row.  A wave
// finds its item's span by bisecting the spans' first_item (uniform: scalar loads), walks the item's rows in CHUNKS -- the bytes
// in front of the first 16-byte boundary of the row, then one aligned 16-byte load each, the last one possibly short -- one chunk
// per lane and step, sums each chunk with packed byte arithmetic (v_sad_u8, v_dot4_u32_u8), hands the lanes' sums through LDS,
// and lane 0 adds the item's two terms, reduced mod M, to the digest's 64-bit accumulators with integer atomics.  The host has
// put a0 and b0 + N * a0 there; k_digest_final reduces mod M and packs.  Every byte a wave reads lies inside a row of a span:
// short chunks are read byte by byte.
//
// Nothing wraps: a chunk's sums are below 2^16; a lane's b term per chunk is below 4080 * DIGEST_PIECE + 2^16 < 2^27 and is
// summed in 64 bits; a_c <= 255 * DIGEST_PIECE < 2^23; (a_c mod M) * (T mod M) < 2^32; an accumulator grows by less than M per
// item and 255 per byte.
//
// Written in the H263_HD style of the other kernels: tests/sim_digest/ runs digest_item and digest_final lane by lane under g++
// (ASan / UBSan) over a buffer of exactly buffer_bytes.
#pragma once

#include "dev_common.h"

#include <vector>

namespace h263mi {

constexpr uint32_t DIGEST_MOD = 65521u;
constexpr uint32_t DIGEST_PIECE = 16384u;                // bytes of one work item at most; a multiple of 16
constexpr uint32_t DIGEST_MAX_ROWS = 64u;                // rows of one work item at most
constexpr uint32_t DIGEST_MAX_SPANS = 65536u;
constexpr uint64_t DIGEST_MAX_BYTES = 1ull << 32;        // one digest covers fewer bytes than this

// a span as the waves see it (digest_table)
struct DigestSpan {
    uint64_t offset, pitch;      // as h263mi_digest_span
    uint64_t tail;               // bytes of the digest's string behind the span's last byte
    uint64_t first_item;         // work items of the spans in front of it
    uint32_t row_bytes, rows, digest;
    uint32_t rows_per_item;      // rows shorter than DIGEST_PIECE: whole rows per item; 0: every row is cut into pieces
};

struct DigestArgs {
    const uint8_t *base;
    const DigestSpan *spans;
    unsigned long long *acc;     // per digest: A, B -- a0 and b0 + (N mod M) * a0 when the launch starts
    uint64_t n_items;
    uint32_t n_spans, pad;
};

struct DigestFinalArgs {
    const unsigned long long *acc;
    uint32_t *out;
    uint32_t n_digests, pad;
};

// what a wave hands between its lanes: every lane's sums, then the sums of eight lanes each
struct DigestLds {
    uint64_t b[64], b8[8];
    uint32_t a[64], a8[8];
};

struct DigestLane {
    uint64_t b;
    uint32_t a;
};

// acc + the four bytes of `word`
H263_HD uint32_t digest_sum4(uint32_t word, uint32_t acc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sad_u8(word, 0u, acc);
#else
    return acc + (word & 0xffu) + ((word >> 8) & 0xffu) + ((word >> 16) & 0xffu) + (word >> 24);
#endif
}

// acc + sum of byte k of `word` * byte k of `weights`
H263_HD uint32_t digest_dot4(uint32_t word, uint32_t weights, uint32_t acc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_udot4(word, weights, acc, false);
#else
    for (int k = 0; k < 4; k++) acc += ((word >> (8 * k)) & 0xffu) * ((weights >> (8 * k)) & 0xffu);
    return acc;
#endif
}

H263_HD void digest_add(unsigned long long *p, unsigned long long v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    *p += v;
#endif
}

// The lane's chunks of one row segment [p, p + len): chunk 0 is the `head` bytes in front of the first 16-byte boundary, chunk
// c >= 1 the 16 bytes behind head + 16 * (c - 1), cut at len.  `behind`: bytes of the item behind the segment.
H263_HD void digest_row(const uint8_t *p, uint32_t len, uint32_t behind, int lane, DigestLane &t)
{
    const uint32_t to_boundary = (16u - (uint32_t)((uintptr_t)p & 15u)) & 15u, head = to_boundary < len ? to_boundary : len;
    const uint32_t chunks = 1u + (len - head + 15u) / 16u;
    for (uint32_t c = (uint32_t)lane; c < chunks; c += 64u) {
        const uint32_t c0 = c ? head + 16u * (c - 1u) : 0u;
        const uint32_t c1 = c ? (c0 + 16u < len ? c0 + 16u : len) : head, n = c1 - c0;
        uint32_t s = 0, w = 0;                              // sum d_j, sum (n - j) * d_j over the chunk
        if (n == 16u) {                                     // (c >= 1: p + c0 is a multiple of 16)
            const uint4 v = *reinterpret_cast<const uint4 *>(p + c0);
            s = digest_sum4(v.x, digest_sum4(v.y, digest_sum4(v.z, digest_sum4(v.w, 0u))));
            w = digest_dot4(v.x, 0x0d0e0f10u, digest_dot4(v.y, 0x090a0b0cu, digest_dot4(v.z, 0x05060708u, digest_dot4(v.w, 0x01020304u, 0u))));
        } else {
            for (uint32_t j = 0; j < n; j++) {
                const uint32_t d = p[c0 + j];
                s += d;
                w += (n - j) * d;
            }
        }
        t.a += s;
        t.b += w + s * (behind + len - c1);
    }
}

// One wave's work: item `item` of the launch.  `each(f)` runs f(lane, lane_state) for the lanes this thread stands for: the one
// of its hardware lane on the GPU, all 64 in turn in the CPU checker.  Everything outside `each` is wave-uniform.
template <class EachLane>
H263_HD void digest_item(const DigestArgs &a, DigestLds &s, uint64_t item, EachLane each)
{
    // the last span with first_item <= item (spans without bytes have no items and are never found)
    uint32_t lo = 0, hi = a.n_spans;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (a.spans[mid].first_item <= item) lo = mid;
        else hi = mid;
    }
    const DigestSpan sp = a.spans[lo];
    const uint32_t q = (uint32_t)(item - sp.first_item);    // (a span has fewer than 2^32 items: digest_table)
    uint32_t row0, nrows, x0, len;
    uint64_t behind_in_span;
    if (sp.rows_per_item) {
        row0 = q * sp.rows_per_item;
        nrows = sp.rows - row0 < sp.rows_per_item ? sp.rows - row0 : sp.rows_per_item;
        x0 = 0;
        len = sp.row_bytes;
        behind_in_span = (uint64_t)(sp.rows - row0 - nrows) * sp.row_bytes;
    } else {
        const uint32_t per_row = (sp.row_bytes - 1u) / DIGEST_PIECE + 1u;
        row0 = q / per_row;
        nrows = 1;
        x0 = (q - row0 * per_row) * DIGEST_PIECE;
        len = sp.row_bytes - x0 < DIGEST_PIECE ? sp.row_bytes - x0 : DIGEST_PIECE;
        behind_in_span = (uint64_t)(sp.rows - 1u - row0) * sp.row_bytes + (sp.row_bytes - x0 - len);
    }
    const uint8_t *const first = a.base + sp.offset + (uint64_t)row0 * sp.pitch + x0;
    each([&](int lane, DigestLane &t) {
        t.a = 0;
        t.b = 0;
        for (uint32_t r = 0; r < nrows; r++) digest_row(first + (uint64_t)r * sp.pitch, len, (nrows - 1u - r) * len, lane, t);
        s.a[lane] = t.a;
        s.b[lane] = t.b;
    });
    wave_fence();
    each([&](int lane, DigestLane &) {
        if (lane < 8) {
            uint32_t a8 = 0;
            uint64_t b8 = 0;
            for (int k = 0; k < 8; k++) a8 += s.a[8 * lane + k], b8 += s.b[8 * lane + k];
            s.a8[lane] = a8;
            s.b8[lane] = b8;
        }
    });
    wave_fence();
    each([&](int lane, DigestLane &) {
        if (lane == 0) {
            uint32_t a_c = 0;
            uint64_t b_c = 0;
            for (int k = 0; k < 8; k++) a_c += s.a8[k], b_c += s.b8[k];
            const uint64_t t_mod = (sp.tail + behind_in_span) % DIGEST_MOD;
            digest_add(a.acc + 2u * (size_t)sp.digest, a_c);
            digest_add(a.acc + 2u * (size_t)sp.digest + 1u, (b_c % DIGEST_MOD + (a_c % DIGEST_MOD) * t_mod) % DIGEST_MOD);
        }
    });
    wave_fence();                                            // (the wave's next item overwrites the sums)
}

H263_HD void digest_final(const DigestFinalArgs &f, uint32_t k)
{
    const uint32_t A = (uint32_t)(f.acc[2u * (size_t)k] % DIGEST_MOD), B = (uint32_t)(f.acc[2u * (size_t)k + 1u] % DIGEST_MOD);
    f.out[k] = B << 16 | A;
}

// The host half: the caller's table checked (include/h263mi.h lists the refusals: false) and turned into what the waves read.
// out_spans (n_spans entries), out_acc (2 * n_digests) and n_items may be null: the check alone.  No device call.
inline bool digest_table(const h263mi_digest_span *spans, uint32_t n_spans, uint32_t n_digests, uint64_t buffer_bytes, bool have_base,
                         uint32_t seed, DigestSpan *out_spans, unsigned long long *out_acc, uint64_t *n_items)
{
    const uint32_t a0 = seed & 0xffffu, b0 = seed >> 16;
    if (!n_digests || (n_spans && !spans) || n_spans > DIGEST_MAX_SPANS || a0 >= DIGEST_MOD || b0 >= DIGEST_MOD) return false;
    uint64_t length = 0;                                     // of the digest of the span before
    for (uint32_t i = 0; i < n_spans; i++) {
        const h263mi_digest_span &sp = spans[i];
        if (sp.reserved || sp.digest >= n_digests || (i && sp.digest < spans[i - 1].digest)) return false;
        if (sp.rows > 1 && sp.pitch < sp.row_bytes) return false;
        if (i && sp.digest != spans[i - 1].digest) length = 0;
        if (!sp.rows || !sp.row_bytes) continue;
        uint64_t end;
        if (__builtin_mul_overflow((uint64_t)(sp.rows - 1u), sp.pitch, &end) || __builtin_add_overflow(end, sp.offset, &end) ||
            __builtin_add_overflow(end, (uint64_t)sp.row_bytes, &end) || end > buffer_bytes || !have_base)
            return false;
        length += (uint64_t)sp.rows * sp.row_bytes;          // (each term and the sum so far below 2^64)
        if (length >= DIGEST_MAX_BYTES) return false;
    }
    if (!out_spans && !out_acc && !n_items) return true;
    // back to front: what lies behind every span in its digest's string, and every digest's length
    std::vector<uint64_t> lengths(out_acc ? n_digests : 0u, 0u);
    uint64_t behind = 0;
    for (uint32_t i = n_spans; i-- > 0;) {
        const h263mi_digest_span &sp = spans[i];
        if (i + 1 < n_spans && sp.digest != spans[i + 1].digest) behind = 0;
        if (out_spans) out_spans[i].tail = behind;
        behind += (uint64_t)sp.rows * sp.row_bytes;
        if (out_acc) lengths[sp.digest] = behind;
    }
    uint64_t items = 0;
    for (uint32_t i = 0; i < n_spans; i++) {
        const h263mi_digest_span &sp = spans[i];
        uint32_t per_item = 0;
        uint64_t n = 0;
        if (sp.rows && sp.row_bytes) {
            if (sp.row_bytes < DIGEST_PIECE) {
                per_item = DIGEST_PIECE / sp.row_bytes < DIGEST_MAX_ROWS ? DIGEST_PIECE / sp.row_bytes : DIGEST_MAX_ROWS;
                n = ((uint64_t)sp.rows + per_item - 1u) / per_item;
            } else {
                n = (uint64_t)sp.rows * ((sp.row_bytes - 1u) / DIGEST_PIECE + 1u);
            }
        }
        if (out_spans) {
            DigestSpan &o = out_spans[i];
            o.offset = sp.offset;
            o.pitch = sp.pitch;
            o.first_item = items;
            o.row_bytes = sp.row_bytes;
            o.rows = sp.rows;
            o.digest = sp.digest;
            o.rows_per_item = per_item;
        }
        items += n;
    }
    if (n_items) *n_items = items;
    if (out_acc)
        for (uint32_t k = 0; k < n_digests; k++) {
            out_acc[2u * (size_t)k] = a0;
            out_acc[2u * (size_t)k + 1u] = b0 + (lengths[k] % DIGEST_MOD) * a0;
        }
    return true;
}

}  // namespace h263mi
