// filter_taps.h -- the tap tables of the bilinear and bicubic resampling (h263mi_filter, include/h263mi.h has the definition):
// HOST ONLY, it computes in binary64 and divides.  h263mi_filter_taps is filter_taps behind its validation; the shapes
// (output_shape.cpp) upload the same tables for k_rgba_filter / k_tensor_filter, and the CPU checker (tests/sim_filter) makes
// them with the same code.
//
// The arithmetic is IEEE binary64 in the order written and must not be contracted into fused multiply-adds: the library and
// the checker are built with -ffp-contract=off, and the pragma below says so to a compiler that honours it.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

namespace h263mi {

constexpr uint32_t FILTER_AREA = 0, FILTER_BILINEAR = 1, FILTER_BICUBIC = 2;      // (H263MI_FILTER_*)
constexpr int FILTER_BITS = 22;                                                   // weights in units of 2^-22

inline double filter_bilinear(double x)
{
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

inline double filter_bicubic(double x)
{
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// entries per output position of in_size -> out_size (sizes 1..65535: at most 2 * ceil(2 * 65535) + 1)
inline uint32_t filter_ksize(uint32_t kind, uint32_t in_size, uint32_t out_size)
{
#pragma STDC FP_CONTRACT OFF
    const double scale = (double)in_size / (double)out_size, fs = scale < 1.0 ? 1.0 : scale;
    const double support = (kind == FILTER_BICUBIC ? 2.0 : 1.0) * fs;
    return 2u * (uint32_t)std::ceil(support) + 1u;
}

// first[X], count[X], coeffs[X * ksize + k] for the out_size positions (ksize = filter_ksize); weights beyond count are zero
inline void filter_taps(uint32_t kind, uint32_t in_size, uint32_t out_size, uint32_t ksize, uint32_t *first, uint32_t *count,
                        int32_t *coeffs)
{
#pragma STDC FP_CONTRACT OFF
    const double scale = (double)in_size / (double)out_size, fs = scale < 1.0 ? 1.0 : scale;
    const double support = (kind == FILTER_BICUBIC ? 2.0 : 1.0) * fs, ss = 1.0 / fs;
    std::vector<double> k(ksize);
    for (uint32_t X = 0; X < out_size; X++) {
        const double center = (X + 0.5) * scale;
        int xmin = (int)(center - support + 0.5), xmax = (int)(center + support + 0.5);      // (truncating; below 2^18)
        if (xmin < 0) xmin = 0;
        if (xmax > (int)in_size) xmax = (int)in_size;
        const int n = xmax - xmin;
        double ww = 0.0;
        for (int i = 0; i < n; i++) {
            const double x = (i + xmin - center + 0.5) * ss;
            k[i] = kind == FILTER_BICUBIC ? filter_bicubic(x) : filter_bilinear(x);
            ww += k[i];
        }
        int32_t *const out = coeffs + (size_t)X * ksize;
        for (int i = 0; i < n; i++) {
            const double v = ww != 0.0 ? k[i] / ww : k[i];
            out[i] = v < 0.0 ? (int32_t)(-0.5 + v * (double)(1 << FILTER_BITS)) : (int32_t)(0.5 + v * (double)(1 << FILTER_BITS));
        }
        for (uint32_t i = (uint32_t)n; i < ksize; i++) out[i] = 0;
        first[X] = (uint32_t)xmin;
        count[X] = (uint32_t)n;
    }
}

// The tables of one shape as the kernels read them (filter_kernel.inl: filter_axes), in 32-bit words: dw (first, count) pairs of
// the columns, dh pairs of the rows -- `first` in picture coordinates: sx / sy added --, then the dw * ksx column weights and
// the dh * ksy row weights.  An axis whose sizes agree is skipped by definition: its table is the identity, one tap of 2^22.
struct FilterTable {
    std::vector<uint32_t> words;
    uint32_t ksx = 0, ksy = 0;
};

inline uint32_t filter_table_ksize(uint32_t kind, uint32_t in_size, uint32_t out_size)
{
    return in_size == out_size ? 1u : filter_ksize(kind, in_size, out_size);
}

// words of the table of sw x sh -> dw x dh
inline uint64_t filter_table_words(uint32_t kind, uint32_t sw, uint32_t sh, uint32_t dw, uint32_t dh)
{
    return 2ull * dw + 2ull * dh + (uint64_t)dw * filter_table_ksize(kind, sw, dw) + (uint64_t)dh * filter_table_ksize(kind, sh, dh);
}

inline FilterTable filter_table(uint32_t kind, uint32_t sx, uint32_t sy, uint32_t sw, uint32_t sh, uint32_t dw, uint32_t dh)
{
    FilterTable t;
    t.ksx = filter_table_ksize(kind, sw, dw);
    t.ksy = filter_table_ksize(kind, sh, dh);
    t.words.assign((size_t)filter_table_words(kind, sw, sh, dw, dh), 0u);
    uint32_t *span = t.words.data();
    int32_t *coeff = reinterpret_cast<int32_t *>(t.words.data() + 2 * ((size_t)dw + dh));
    const uint32_t in[2] = {sw, sh}, out[2] = {dw, dh}, at[2] = {sx, sy}, ks[2] = {t.ksx, t.ksy};
    for (int axis = 0; axis < 2; axis++) {
        const uint32_t n = out[axis];
        std::vector<uint32_t> first(n), count(n, 1u);
        if (in[axis] == n) {
            for (uint32_t X = 0; X < n; X++) first[X] = X, coeff[X] = 1 << FILTER_BITS;
        } else {
            filter_taps(kind, in[axis], n, ks[axis], first.data(), count.data(), coeff);
        }
        for (uint32_t X = 0; X < n; X++) span[2 * X] = first[X] + at[axis], span[2 * X + 1] = count[X];
        span += 2 * (size_t)n;
        coeff += (size_t)n * ks[axis];
    }
    return t;
}

}  // namespace h263mi
