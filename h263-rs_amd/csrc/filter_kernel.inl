// filter_kernel.inl -- k_rgba_filter, k_tensor_filter: a source window of the full-size RGBA resampled into a destination
// rectangle of the W' x H' output with Pillow's bilinear or bicubic filter (h263mi_filter, ABI 7), stored as RGBA or as the
// normalised planar tensor of h263mi_tensor_out.
//
// The contract (include/h263mi.h): two passes of 22-bit fixed-point taps (filter_taps.h makes the tables on the host),
//     horizontal   t[j][X][c]   = clamp((2^21 + sum_i kx[X][i] * P[j][fx(X) + i][c]) >> 22, 0, 255)      the first rounding
//     vertical     out[Y][X][c] = clamp((2^21 + sum_j ky[Y][j] * t[fy(Y) + j][X][c]) >> 22, 0, 255)      the second rounding
// The passes cannot be fused into one weighted sum: the 8-bit rounding and the clamp between them are part of the result.  But
// the intermediate picture t never reaches memory: a wave = 64 output columns x FILTER_ROWS output rows walks the source rows
// that its rows' vertical taps cover, [fy(Y0), fy(Y1-1) + ny(Y1-1)), ONCE.  Per source row it stages the pixels that its 64
// columns' horizontal taps cover into LDS in chunks of 256 (16-byte loads where the picture's rows are 16-byte aligned; the
// chunk starts at a multiple of 4 in picture coordinates, so a window with an odd sx is loaded aligned all the same), every lane
// sums its column's taps in int32 and rounds and clamps to three bytes -- the horizontal pass of that row --, and adds
// ky * value into one int32 accumulator per channel for each of the wave's output rows whose taps hold that source row.  A tap
// window of thousands of rows or columns (1080p -> 1 x 1) takes no more registers or LDS than a small one.  255 * sum |k| + 2^21
// stays below 2^31 for every row of every table (h263mi_filter_taps documents it, tests/test_filter.py checks it): int32 holds
// every sum.  A pass whose sizes agree is skipped by definition: its table is the identity (one tap of 2^22 per position),
// which the same arithmetic hands through bit for bit.
//
// The horizontal coefficient rows of a wave's 64 columns are held in LDS, lane-major per tap (no bank conflict), where a row has at
// most FILTER_LDS_TAPS entries -- 1080p -> 224 bicubic has 37 --; longer rows are read from the table, which every wave of a
// picture column shares (L2).  LDS per workgroup: 3 KB hand-off + 10 KB coefficients.
//
// One instantiation covers the framed and the unframed case: the unframed output is the framing with a whole rectangle.  The
// launch shape, the pad / keep_outside rules and the stores are those of k_rgba_resize_framed / k_tensor_resize_framed
// (resize_kernel.inl: FrameRect; tensor_resize_kernel.inl: tensor_value, tensor_phase_store32, framed_phase_store16 -- the
// same functions): one wave per workgroup, no barrier, blockIdx.y = picture, blockIdx.z = segment of 64 output columns,
// blockIdx.x = band of FILTER_ROWS output rows in XCD order.
//
// Written in the H263_HD style of the other kernels: tests/sim_filter/ runs filter_rgba_item and filter_tensor_item lane by
// lane under g++ (ASan / UBSan), also with the two mutants of mutants.h.
#pragma once

#include "mutants.h"
#include "tensor_resize_kernel.inl"

namespace h263mi {

constexpr uint32_t FILTER_ROWS = 4;          // output rows per wave
constexpr uint32_t FILTER_CHUNK = 256;       // source columns per LDS hand-off (4 per lane)
constexpr uint32_t FILTER_LDS_TAPS = 40;     // horizontal coefficient rows up to this length are held in LDS
constexpr int FILTER_SHIFT = 22;             // (filter_taps.h: FILTER_BITS)

// one output position of an axis: it reads the source positions [first, first + count) -- `first` in PICTURE coordinates (the
// window's sx / sy added)
struct FilterSpan {
    uint32_t first, count;
};

struct FilterAxis {
    const FilterSpan *span;      // one per output position of the rectangle
    const int32_t *coeff;        // coeff[X * ksize + k]: the weight of source position first + k, zero beyond count
    uint32_t ksize;
};

struct FilterArgs {
    const uint8_t *src;          // full-size RGBA, picture p at + p * w*h*4, rows w*4 bytes apart
    uint8_t *const *dst;         // DEVICE array: picture p's output at dst[p]; nullptr = skip p
    FilterAxis x, y;             // the tables of sw -> dw and sh -> dh
    uint32_t w, h;               // the full-size picture
    uint32_t dw, dh;             // the destination rectangle's size (its place: f.dx, f.dy)
    uint32_t pitch;              // RGBA: bytes between output rows
    uint32_t bands;              // ceil(f.ch / FILTER_ROWS)
    uint32_t chunk;              // bands per picture and XCD: ceil(bands / 8)
    uint32_t n_pictures;
    FrameRect f;                 // the W' x H' output around the rectangle, pad and keep
};

// the axes of a table that lies at `base` (filter_taps.h: filter_table has the layout)
H263_HD void filter_axes(const void *base, uint32_t dw, uint32_t dh, uint32_t ksx, uint32_t ksy, FilterAxis &x, FilterAxis &y)
{
    x.span = static_cast<const FilterSpan *>(base);
    y.span = x.span + dw;
    x.coeff = reinterpret_cast<const int32_t *>(y.span + dh);
    y.coeff = x.coeff + (size_t)dw * ksx;
    x.ksize = ksx;
    y.ksize = ksy;
}

struct TensorFilterArgs {
    FilterArgs fl;
    TensorArgs t;                // scale, bias, dtype, bgr, strides; t.r is not used
};

// what a filter launch must hold before a wave runs: tables, a rectangle that is not empty and lies inside the output, a source
// picture
inline bool filter_args_ok(const FilterArgs &a)
{
    const FrameRect &f = a.f;
    return a.src && a.dst && a.x.span && a.x.coeff && a.y.span && a.y.coeff && a.x.ksize && a.y.ksize && a.w && a.h && a.dw && a.dh &&
           f.cw && f.ch && f.keep <= 1 && f.dx <= f.cw && a.dw <= f.cw - f.dx && f.dy <= f.ch && a.dh <= f.ch - f.dy && a.n_pictures <= 65535;
}

// the launches of k_rgba_filter and k_tensor_filter over the f.cw x f.ch output (HOST)
inline bool filter_rgba_plan(FilterArgs &a, LaunchDims &d)
{
    if (!filter_args_ok(a)) return false;
    d = band_grid(a.f.ch, FILTER_ROWS, a.n_pictures, (a.f.cw + 63) / 64, a.bands, a.chunk);
    return true;
}

inline bool filter_tensor_plan(TensorFilterArgs &a, LaunchDims &d) { return a.t.dtype <= TENSOR_BF16 && filter_rgba_plan(a.fl, d); }

struct FilterLds {
    ResizeLds hand;              // v[0][0..255]: the staged pixels of a chunk; then v[c][lane]: the tensor's 16-bit hand-off
    int32_t kx[FILTER_LDS_TAPS][64];
};

// the vertical accumulator: int32 in the product (the single-rounding mutant carries 44 fraction bits)
template <bool Wide>
struct FilterAcc {
    typedef int32_t type;
};
template <>
struct FilterAcc<true> {
    typedef int64_t type;
};
typedef FilterAcc<mutants::kFilterSingleRounding>::type filter_acc_t;

// what a lane keeps across a band
struct FilterLane {
    FilterSpan cs;                       // its column's horizontal taps
    int32_t h[3];                        // the horizontal sums of the source row at hand
    filter_acc_t acc[FILTER_ROWS][3];
};

struct TensorFilterLane {
    FilterLane fl;
    TensorLane t;
};

H263_HD int32_t filter_clamp8(int64_t v) { return (int32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// the horizontal pass's result for one channel: the first rounding
H263_HD int32_t filter_round_h(int32_t sum)
{
    if (mutants::kFilterSingleRounding) return sum;
    const int32_t v = (sum + (1 << (FILTER_SHIFT - 1))) >> FILTER_SHIFT;
    if (mutants::kFilterNoClamp) return v & 0xff;
    return filter_clamp8(v);
}

// the vertical pass's result: the second rounding
H263_HD uint32_t filter_round_v(filter_acc_t acc)
{
    const int shift = mutants::kFilterSingleRounding ? 2 * FILTER_SHIFT : FILTER_SHIFT;
    return (uint32_t)filter_clamp8((int64_t)(acc + ((filter_acc_t)1 << (shift - 1))) >> shift);
}

// One source row's staging: the lane's 4 pixels c + 4*lane .. +3 of row `row` into LDS (c is a multiple of 4: with w a multiple
// of 4 too, they are one aligned 16-byte load inside the row)
H263_HD void filter_phase_stage(const FilterArgs &a, FilterLds &s, int lane, const uint8_t *row, uint32_t c, uint32_t c_end)
{
    const uint32_t x = c + 4u * (uint32_t)lane;
    if (x >= c_end) return;              // (what no tap reads is not staged)
    uint32_t *const out = &s.hand.v[0][4 * lane];
    if ((a.w & 3u) == 0) {
        const uint4 p = *reinterpret_cast<const uint4 *>(row + (size_t)x * 4u);
        out[0] = p.x, out[1] = p.y, out[2] = p.z, out[3] = p.w;
    } else {
        for (uint32_t e = 0; e < 4; e++)
            if (x + e < c_end) out[e] = *reinterpret_cast<const uint32_t *>(row + (size_t)(x + e) * 4u);
    }
}

// The lane's taps that lie in the chunk [c, c + 256), weighed into its horizontal sums.  kx: its coefficient row in the table
// (used where the rows are not in LDS)
H263_HD void filter_phase_horizontal(const FilterLds &s, FilterLane &t, int lane, const int32_t *kx, bool in_lds, uint32_t c)
{
    const uint32_t b = t.cs.first > c ? t.cs.first : c;
    const uint32_t e0 = t.cs.first + t.cs.count, e1 = c + FILTER_CHUNK, e = e0 < e1 ? e0 : e1;
    for (uint32_t i = b; i < e; i++) {
        const uint32_t k = i - t.cs.first;
        const int32_t wt = in_lds ? s.kx[k][lane] : kx[k];
        const uint32_t px = s.hand.v[0][i - c];
        t.h[0] += wt * (int32_t)(px & 0xffu);
        t.h[1] += wt * (int32_t)((px >> 8) & 0xffu);
        t.h[2] += wt * (int32_t)((px >> 16) & 0xffu);
    }
}

// Both passes for the rectangle's rows [Ya, Yb) (output coordinates, inside one band that starts at Y0) and its columns
// [xa, xb] of the segment that starts at X0: afterwards lane's acc[Y - Y0][c] holds the vertical sums of its column.
template <class Lane, class EachLane, class Get>
H263_HD void filter_passes(const FilterArgs &a, FilterLds &s, const uint8_t *pic_src, uint32_t Y0, uint32_t Ya, uint32_t Yb, uint32_t X0,
                           uint32_t xa, uint32_t xb, EachLane each, Get get)
{
    const FrameRect &f = a.f;
    const uint32_t ksx = a.x.ksize, ksy = a.y.ksize;
    const bool in_lds = ksx <= FILTER_LDS_TAPS;
    // the lanes' columns, their coefficient rows
    each([&](int lane, Lane &L) {
        FilterLane &t = get(L);
        const uint32_t X = X0 + (uint32_t)lane;
        const bool valid = X >= xa && X <= xb;
        t.cs = valid ? a.x.span[X - f.dx] : FilterSpan{0, 0};
#pragma unroll
        for (uint32_t r = 0; r < FILTER_ROWS; r++) t.acc[r][0] = t.acc[r][1] = t.acc[r][2] = 0;
        if (valid && in_lds) {
            const int32_t *kx = a.x.coeff + (size_t)(X - f.dx) * ksx;
            for (uint32_t k = 0; k < ksx; k++) s.kx[k][lane] = kx[k];
        }
    });
    // (a lane reads back its own coefficients only: no fence)
    const FilterSpan ca = a.x.span[xa - f.dx], cb = a.x.span[xb - f.dx];
    const uint32_t c0 = ca.first & ~3u, c_end = cb.first + cb.count;
    // the band's rows: their vertical taps (wave-uniform)
    FilterSpan ys[FILTER_ROWS];
#pragma unroll
    for (uint32_t r = 0; r < FILTER_ROWS; r++) {
        const uint32_t Y = Y0 + r;
        ys[r] = Y >= Ya && Y < Yb ? a.y.span[Y - f.dy] : FilterSpan{0, 0};
    }
    const FilterSpan ra = a.y.span[Ya - f.dy], rb = a.y.span[Yb - 1u - f.dy];
    const uint32_t j0 = ra.first, j1 = rb.first + rb.count;
    for (uint32_t j = j0; j < j1; j++) {
        const uint8_t *const row = pic_src + (size_t)j * a.w * 4u;
        each([&](int lane, Lane &L) { get(L).h[0] = get(L).h[1] = get(L).h[2] = 0; });
        for (uint32_t c = c0; c < c_end; c += FILTER_CHUNK) {
            each([&](int lane, Lane &) { filter_phase_stage(a, s, lane, row, c, c_end); });
            wave_fence();
            each([&](int lane, Lane &L) {
                const uint32_t X = X0 + (uint32_t)lane;
                if (X < xa || X > xb) return;
                filter_phase_horizontal(s, get(L), lane, a.x.coeff + (size_t)(X - f.dx) * ksx, in_lds, c);
            });
            wave_fence();                                     // (the next chunk's pixels overwrite these)
        }
        // the weights of this source row in the band's output rows (wave-uniform: scalar loads)
        int32_t kv[FILTER_ROWS];
#pragma unroll
        for (uint32_t r = 0; r < FILTER_ROWS; r++) {
            const bool holds = j >= ys[r].first && j - ys[r].first < ys[r].count;
            kv[r] = holds ? a.y.coeff[(size_t)(Y0 + r - f.dy) * ksy + (j - ys[r].first)] : 0;
        }
        each([&](int lane, Lane &L) {
            FilterLane &t = get(L);
            for (int ch = 0; ch < 3; ch++) {
                const int32_t v = filter_round_h(t.h[ch]);
#pragma unroll
                for (uint32_t r = 0; r < FILTER_ROWS; r++) t.acc[r][ch] += (filter_acc_t)kv[r] * v;
            }
        });
    }
}

// what the items share: the segment's columns and the band's rows against the rectangle
struct FilterWave {
    uint32_t X0, X1, xa, xb, Y0, Y1, Ya, Yb;
    bool cols_in, any_in;
};

H263_HD FilterWave filter_wave(const FilterArgs &a, uint32_t band, uint32_t seg)
{
    const FrameRect &f = a.f;
    FilterWave v;
    v.X0 = seg * 64u;
    v.X1 = (v.X0 + 64u < f.cw ? v.X0 + 64u : f.cw) - 1u;
    v.cols_in = frame_columns(f, a.dw, v.X0, v.X1, v.xa, v.xb);
    v.Y0 = band * FILTER_ROWS;
    v.Y1 = v.Y0 + FILTER_ROWS < f.ch ? v.Y0 + FILTER_ROWS : f.ch;
    v.Ya = v.Y0 > f.dy ? v.Y0 : f.dy;
    v.Yb = v.Y1 < f.dy + a.dh ? v.Y1 : f.dy + a.dh;
    v.any_in = v.cols_in && v.Ya < v.Yb;
    return v;
}

// One wave's work: the 64 output columns of segment `seg` in band `band` of picture `pic`, as RGBA.  `each(f)` runs
// f(lane, lane_state) for the lanes this thread stands for: the one of its hardware lane on the GPU, all 64 in turn in the CPU
// checker.  Everything outside `each` is wave-uniform.
template <class EachLane>
H263_HD void filter_rgba_item(const FilterArgs &a, FilterLds &s, uint32_t band, uint32_t seg, uint32_t pic, EachLane each)
{
    const FrameRect &f = a.f;
    uint8_t *const pic_dst = a.dst[pic];
    if (!pic_dst) return;                                     // a stream with nothing to render: untouched
    const uint8_t *const pic_src = a.src + (size_t)pic * a.w * a.h * 4u;
    const FilterWave v = filter_wave(a, band, seg);
    if (!v.any_in && f.keep) return;
    if (v.any_in)
        filter_passes<FilterLane>(a, s, pic_src, v.Y0, v.Ya, v.Yb, v.X0, v.xa, v.xb, each, [](FilterLane &t) -> FilterLane & { return t; });
#pragma unroll
    for (uint32_t r = 0; r < FILTER_ROWS; r++) {
        const uint32_t Y = v.Y0 + r;
        if (Y >= v.Y1) break;
        const bool row_in = v.any_in && Y >= v.Ya && Y < v.Yb;
        if (!row_in && f.keep) continue;
        each([&](int lane, FilterLane &t) {
            const uint32_t X = v.X0 + (uint32_t)lane;
            if (X > v.X1) return;
            const bool inside = row_in && X >= v.xa && X <= v.xb;
            if (!inside && f.keep) return;
            uint32_t px = f.pad;
            if (inside) px = filter_round_v(t.acc[r][0]) | (filter_round_v(t.acc[r][1]) << 8) | (filter_round_v(t.acc[r][2]) << 16);
            *reinterpret_cast<uint32_t *>(pic_dst + (size_t)Y * a.pitch + (size_t)X * 4u) = px | 0xff000000u;
        });
    }
}

// ... as the normalised planar tensor: every u, the pad colour included, goes through tensor_value and the stores of
// k_tensor_resize_framed
template <class EachLane>
H263_HD void filter_tensor_item(const TensorFilterArgs &ta, FilterLds &s, uint32_t band, uint32_t seg, uint32_t pic, EachLane each)
{
    const FilterArgs &a = ta.fl;
    const TensorArgs &tn = ta.t;
    const FrameRect &f = a.f;
    uint8_t *const pic_dst = a.dst[pic];
    if (!pic_dst) return;                                     // a stream with nothing to render: untouched
    const uint8_t *const pic_src = a.src + (size_t)pic * a.w * a.h * 4u;
    const FilterWave v = filter_wave(a, band, seg);
    if (!v.any_in && f.keep) return;
    if (v.any_in) {
        filter_passes<TensorFilterLane>(a, s, pic_src, v.Y0, v.Ya, v.Yb, v.X0, v.xa, v.xb, each,
                                        [](TensorFilterLane &t) -> FilterLane & { return t.fl; });
        wave_fence();                                         // (the values below overwrite the staged pixels)
    }
#pragma unroll
    for (uint32_t r = 0; r < FILTER_ROWS; r++) {
        const uint32_t Y = v.Y0 + r;
        if (Y >= v.Y1) break;
        const bool row_in = v.any_in && Y >= v.Ya && Y < v.Yb;
        if (!row_in && f.keep) continue;
        // the columns this row writes
        const uint32_t wa = f.keep ? v.xa : v.X0, wb = f.keep ? v.xb : v.X1;
        auto value = [&](int lane, TensorFilterLane &t) {
            const uint32_t X = v.X0 + (uint32_t)lane;
            const bool inside = row_in && X >= v.xa && X <= v.xb;
            for (int c = 0; c < 3; c++) {
                const uint32_t u = inside ? filter_round_v(t.fl.acc[r][c]) : (f.pad >> (8 * c)) & 0xffu;
                t.t.v[c] = tensor_bits_of(tensor_value(u, tn.scale[c], tn.bias[c]));
            }
        };
        if (tn.dtype == TENSOR_F32) {
            each([&](int lane, TensorFilterLane &t) {
                const uint32_t X = v.X0 + (uint32_t)lane;
                value(lane, t);
                tensor_phase_store32(tn, t.t, pic_dst, X, Y, X >= wa && X <= wb);
            });
        } else {
            each([&](int lane, TensorFilterLane &t) {
                value(lane, t);
                for (int c = 0; c < 3; c++) s.hand.v[c][lane] = t.t.v[c];
            });
            wave_fence();
            each([&](int lane, TensorFilterLane &t) { framed_phase_store16(tn, s.hand, t.t, lane, pic_dst, v.X0 + (uint32_t)lane, wa, wb, Y); });
            wave_fence();                                     // (the next row's values overwrite these)
        }
    }
}

}  // namespace h263mi
