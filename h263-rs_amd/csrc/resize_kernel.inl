// resize_kernel.inl -- k_rgba_resize: full-size RGBA -> W' x H' by area averaging (h263mi_rgba_resize, ABI 7).
//
// The contract (include/h263mi.h): output column X covers [X*w, (X+1)*w) and source column i covers [i*W', (i+1)*W') in
// units of 1 / (w*W') of a picture width; ox(X, i) is the length of their intersection (sum over i: w), oy(Y, j) the same for
// rows (sum over j: h), and
//     out[Y][X][c] = (sum_j sum_i oy(Y, j) * ox(X, i) * P[j][i][c] + floor(w*h / 2)) div (w*h),   alpha 255.
// The filter is separable: an output column reads `count` source columns from `first` on, the first with weight w_first,
// the last with w_last, every one between with W' (ResizeSpan; the same for rows with H').  The spans of a geometry are a
// small table made on the host (resize_spans: it divides, the device does not -- DESIGN section 3).
//
// One wave per workgroup, no barrier: a wave = 64 output columns (one per lane) x RESIZE_ROWS output rows of one picture;
// blockIdx.y = picture, blockIdx.z = column segment, blockIdx.x = band in XCD order (output_kernels.hip: k_rgba_resize).
// Per output row it walks the source columns its 64 columns cover in chunks of 256: each lane sums 4 adjacent source pixels
// down the row's source rows (coalesced 16-byte loads when a row is 16-byte aligned), the wave hands the 256 column sums
// through LDS, and each lane weighs the ones its output column covers.  Source pixels are read once per output row that
// covers them: twice at most when shrinking (the edge rows), and once per output row when enlarging.
//
// Written in the H263_HD style of the other kernels: tests/sim_resize/ runs resize_item lane by lane under g++
// (ASan / UBSan), with the same ResizeArgs and the same arithmetic.
#pragma once

#include "band_launch.h"
#include "dev_common.h"

namespace h263mi {

constexpr uint32_t RESIZE_ROWS = 4;        // output rows per wave
constexpr uint32_t RESIZE_CHUNK = 256;     // source columns per LDS hand-off (4 per lane)

// one output column (row) of a geometry: source columns (rows) [first, first + count), weights w_first, W' ..., w_last
// (count == 1: w_first alone, which is then w -- the whole output span lies in one source pixel)
struct ResizeSpan {
    uint32_t first, count, w_first, w_last;
};

struct ResizeArgs {
    const uint8_t *src;          // full-size RGBA, picture p at + p * w*h*4, rows w*4 bytes apart
    uint8_t *const *dst;         // DEVICE array: picture p's W' x H' at dst[p], rows `pitch` bytes apart; nullptr = skip p
    const ResizeSpan *cols;      // W' entries
    const ResizeSpan *rows;      // H' entries
    uint32_t w, h, ow, oh;
    uint32_t pitch;              // (H'-1) * pitch + 4W' < 2^32 (h263mi_rgba_resize_extent)
    uint32_t bands;              // ceil(H' / RESIZE_ROWS): bands of output rows per picture
    uint32_t chunk;              // bands per picture and XCD: ceil(bands / 8)
    uint32_t d;                  // w*h (< 2^32: layout_fits)
    float inv_d;                 // 1.0f / d, rounded to nearest
    uint32_t n_pictures;
};

// the launch of k_rgba_resize (HOST: bands, chunk and the grid; nothing is refused)
inline bool resize_plan(ResizeArgs &a, LaunchDims &d)
{
    d = band_grid(a.oh, RESIZE_ROWS, a.n_pictures, (a.ow + 63) / 64, a.bands, a.chunk);
    return true;
}

// HOST ONLY (it divides): the spans of the W' output columns of a w-wide picture (rows: call it with h, H')
inline void resize_spans(uint32_t w, uint32_t ow, ResizeSpan *out)
{
    // (X+1) * w <= W' * w <= 65535^2 < 2^32: every product below fits 32 bits
    for (uint32_t X = 0; X < ow; X++) {
        const uint32_t lo = X * w, hi = lo + w;
        const uint32_t first = lo / ow, last = (hi - 1) / ow;
        const uint32_t first_end = (first + 1) * ow, last_begin = last * ow;
        out[X].first = first;
        out[X].count = last - first + 1;
        out[X].w_first = (hi < first_end ? hi : first_end) - lo;
        out[X].w_last = hi - (lo > last_begin ? lo : last_begin);
    }
}

// weight of the k-th of a span's source columns (rows); `inner` = W' (H')
H263_HD uint32_t resize_weight(const ResizeSpan &s, uint32_t k, uint32_t inner)
{
    return k == 0 ? s.w_first : (k + 1 == s.count ? s.w_last : inner);
}

// (num + floor(d / 2)) div d for num <= 255 * d -- exact, without an integer division instruction.
//
// Let n = num + floor(d/2) and x = n / d, so 0 <= x <= 255.5, and d = w*h < 2^30 (layout_fits), n < 2^38.  The estimate is
// f = fl(fl(n) * inv_d) with inv_d = fl(1/d): three roundings of at most 2^-24 relative each (a truncating conversion of n
// counts as 2^-23), so f = x * (1 + e) with |e| <= 2^-23 + 2 * 2^-24 + 2^-46 < 2^-21, and |f - x| <= 255.5 * 2^-21 < 2^-12.
// Hence q0 = trunc(f) differs from q = floor(x) by at most one: q0 = q - 1 only if x lies within 2^-12 above an integer,
// q0 = q + 1 only if it lies within 2^-12 below one (x = 255.5 - 2^-13 gives q0 <= 256, so q0 * d <= 2^38 fits).  One integer
// multiply r = n - q0 * d and a compare fix it: r < 0 -> q0 - 1, r >= d -> q0 + 1.  tests/sim_resize checks n = q*d - 1, q*d,
// q*d + d/2 for every q of 0..255 at the largest d that the library accepts.
H263_HD uint32_t resize_div(uint64_t n, uint32_t d, float inv_d)
{
    uint32_t q = (uint32_t)((float)n * inv_d);
    const int64_t r = (int64_t)n - (int64_t)((uint64_t)q * d);
    if (r < 0) q--;
    else if (r >= (int64_t)d) q++;
    return q;
}

// what a wave hands between its lanes: the 256 column sums of one chunk, channel-major
struct ResizeLds {
    uint32_t v[3][RESIZE_CHUNK];
};

// what a lane keeps across the phases of one output row
struct ResizeLane {
    uint64_t acc[3];
};

H263_HD void resize_unpack_add(uint32_t px, uint32_t wt, uint32_t *v)
{
    v[0] += wt * (px & 0xffu);
    v[1] += wt * ((px >> 8) & 0xffu);
    v[2] += wt * ((px >> 16) & 0xffu);
}

// Phase 1: lane's 4 source columns c0 + 4*lane .. +3 summed down the output row's source rows (weights oy), into LDS.
// The sums are at most 255 * sum_j oy = 255 * h < 2^24.
H263_HD void resize_phase_vertical(const ResizeArgs &a, ResizeLds &s, int lane, const uint8_t *pic_src, const ResizeSpan &rs,
                                   uint32_t c0, uint32_t c_end)
{
    uint32_t v[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    const uint32_t x = c0 + 4u * (uint32_t)lane;
    if (x < c_end) {
        // (c0 is a multiple of 4: with w a multiple of 4 too, the lane's 4 pixels are one aligned 16-byte load inside the row)
        const bool wide = (a.w & 3u) == 0;
        for (uint32_t k = 0; k < rs.count; k++) {
            const uint32_t wt = resize_weight(rs, k, a.oh);
            const uint8_t *row = pic_src + (size_t)(rs.first + k) * a.w * 4u;
            if (wide) {
                const uint4 p = *reinterpret_cast<const uint4 *>(row + (size_t)x * 4u);
                resize_unpack_add(p.x, wt, v[0]);
                resize_unpack_add(p.y, wt, v[1]);
                resize_unpack_add(p.z, wt, v[2]);
                resize_unpack_add(p.w, wt, v[3]);
            } else {
                for (uint32_t e = 0; e < 4; e++)
                    if (x + e < a.w) resize_unpack_add(*reinterpret_cast<const uint32_t *>(row + (size_t)(x + e) * 4u), wt, v[e]);
            }
        }
    }
    for (uint32_t e = 0; e < 4; e++)
        for (int c = 0; c < 3; c++) s.v[c][4 * lane + e] = v[e][c];
}

// Phase 2: the lane's output column X weighs the column sums of the chunk [c0, c0 + 256) that it covers (weights ox)
H263_HD void resize_phase_horizontal(const ResizeArgs &a, const ResizeLds &s, ResizeLane &t, const ResizeSpan &cs, bool valid,
                                     uint32_t c0)
{
    if (!valid) return;
    const uint32_t b = cs.first > c0 ? cs.first : c0;
    const uint32_t e0 = cs.first + cs.count, e1 = c0 + RESIZE_CHUNK, e = e0 < e1 ? e0 : e1;
    for (uint32_t i = b; i < e; i++) {
        const uint64_t wt = resize_weight(cs, i - cs.first, a.ow);
        for (int c = 0; c < 3; c++) t.acc[c] += wt * s.v[c][i - c0];
    }
}

// Phase 3: round, divide and store the lane's pixel of row Y
H263_HD void resize_phase_store(const ResizeArgs &a, const ResizeLane &t, uint8_t *pic_dst, uint32_t X, uint32_t Y, bool valid)
{
    if (!valid) return;
    const uint32_t half = a.d >> 1;
    const uint32_t r = resize_div(t.acc[0] + half, a.d, a.inv_d), g = resize_div(t.acc[1] + half, a.d, a.inv_d),
                   b = resize_div(t.acc[2] + half, a.d, a.inv_d);
    *reinterpret_cast<uint32_t *>(pic_dst + (size_t)Y * a.pitch + (size_t)X * 4u) = r | (g << 8) | (b << 16) | 0xff000000u;
}

// One wave's work: the 64 output columns of segment `seg` in band `band` of picture `pic`.  `each(f)` runs f(lane, lane_state) for the lanes this thread
// stands for: the one of its hardware lane on the GPU, all 64 in turn in the CPU checker.  Everything outside `each` is
// wave-uniform.
template <class EachLane>
H263_HD void resize_item(const ResizeArgs &a, ResizeLds &s, uint32_t band, uint32_t seg, uint32_t pic, EachLane each)
{
    uint8_t *const pic_dst = a.dst[pic];
    if (!pic_dst) return;                                     // a stream with nothing to render: untouched
    const uint8_t *const pic_src = a.src + (size_t)pic * a.d * 4u;
    const uint32_t X0 = seg * 64u, X1 = (X0 + 64u < a.ow ? X0 + 64u : a.ow) - 1u;
    const uint32_t c0 = a.cols[X0].first & ~3u, c_end = a.cols[X1].first + a.cols[X1].count;
    const uint32_t Y0 = band * RESIZE_ROWS, Y1 = Y0 + RESIZE_ROWS < a.oh ? Y0 + RESIZE_ROWS : a.oh;
    for (uint32_t Y = Y0; Y < Y1; Y++) {
        const ResizeSpan rs = a.rows[Y];
        each([&](int lane, ResizeLane &t) { t.acc[0] = t.acc[1] = t.acc[2] = 0; });
        for (uint32_t c = c0; c < c_end; c += RESIZE_CHUNK) {
            each([&](int lane, ResizeLane &) { resize_phase_vertical(a, s, lane, pic_src, rs, c, c_end); });
            wave_fence();
            each([&](int lane, ResizeLane &t) {
                const uint32_t X = X0 + (uint32_t)lane;
                const bool valid = X <= X1;
                resize_phase_horizontal(a, s, t, valid ? a.cols[X] : a.cols[X1], valid, c);
            });
            wave_fence();                                     // (the next chunk's column sums overwrite these)
        }
        each([&](int lane, ResizeLane &t) { resize_phase_store(a, t, pic_dst, X0 + (uint32_t)lane, Y, X0 + (uint32_t)lane <= X1); });
    }
}

// ---------------------------------------------------------------------------------------
// k_rgba_resize_framed: a source window of the picture into a destination rectangle of the W' x H' output (h263mi_framing).
//
// FramedResizeArgs::r describes the resize INSIDE the rectangle: r.ow x r.oh is dw x dh, the span tables have dw and dh
// entries made over sw -> dw and sh -> dh with `first` offset by sx / sy, and r.d is sw*sh -- so phases 1 and 2 above run
// unchanged on the full-size scratch at its real row stride (r.w; the 16-byte load path stays keyed on it: c0 = first & ~3
// may start left of the window, on columns that are read, inside the picture, and never weighted).  The launch shape is that
// of the W' x H' output (cw x ch here): a wave still owns 64 output columns x RESIZE_ROWS rows of it.  A row or a segment
// wholly outside the rectangle skips phases 1 and 2 and stores the pad colour, or nothing with `keep`; lanes outside the
// rectangle in a mixed wave carry the pad colour.  Every byte is written once.
// ---------------------------------------------------------------------------------------
struct FrameRect {
    uint32_t cw, ch;             // the W' x H' output that the launch covers
    uint32_t dx, dy;             // where the r.ow x r.oh rectangle lies in it: dx + r.ow <= cw, dy + r.oh <= ch
    uint32_t pad;                // R | G << 8 | B << 16: the colour outside the rectangle
    uint32_t keep;               // 1: nothing outside the rectangle is written
};

struct FramedResizeArgs {
    ResizeArgs r;                // pitch, dst, bands and chunk are the OUTPUT's (bands = ceil(ch / RESIZE_ROWS))
    FrameRect f;
};

// what a framed launch must hold before a wave runs: a rectangle that is not empty and lies inside the output
inline bool frame_rect_ok(const ResizeArgs &r, const FrameRect &f)
{
    return r.ow && r.oh && f.cw && f.ch && f.keep <= 1 && f.dx <= f.cw && r.ow <= f.cw - f.dx && f.dy <= f.ch && r.oh <= f.ch - f.dy;
}

// the launch of a framed resize over the cw x ch output (HOST; r: the ResizeArgs inside the launch's arguments)
inline bool framed_plan(ResizeArgs &r, const FrameRect &f, LaunchDims &d)
{
    if (r.n_pictures > 65535 || !frame_rect_ok(r, f)) return false;
    d = band_grid(f.ch, RESIZE_ROWS, r.n_pictures, (f.cw + 63) / 64, r.bands, r.chunk);
    return true;
}

inline bool framed_resize_plan(FramedResizeArgs &a, LaunchDims &d) { return framed_plan(a.r, a.f, d); }

// the columns of the rectangle that segment [X0, X1] holds: [xa, xb], empty (false) when xa > xb
H263_HD bool frame_columns(const FrameRect &f, uint32_t dw, uint32_t X0, uint32_t X1, uint32_t &xa, uint32_t &xb)
{
    xa = X0 > f.dx ? X0 : f.dx;
    xb = X1 < f.dx + dw - 1u ? X1 : f.dx + dw - 1u;
    return xa <= xb;
}

// phases 1 and 2 of output row Y (a row of the rectangle) for the rectangle's columns [xa, xb] of a segment that starts at X0
template <class Lane, class EachLane, class Sums>
H263_HD void framed_phases(const ResizeArgs &a, const FrameRect &f, ResizeLds &s, const uint8_t *pic_src, uint32_t Y, uint32_t X0,
                           uint32_t xa, uint32_t xb, EachLane each, Sums sums)
{
    const ResizeSpan rs = a.rows[Y - f.dy];
    const ResizeSpan &ca = a.cols[xa - f.dx], &cb = a.cols[xb - f.dx];
    const uint32_t c0 = ca.first & ~3u, c_end = cb.first + cb.count;
    for (uint32_t c = c0; c < c_end; c += RESIZE_CHUNK) {
        each([&](int lane, Lane &) { resize_phase_vertical(a, s, lane, pic_src, rs, c, c_end); });
        wave_fence();
        each([&](int lane, Lane &t) {
            const uint32_t X = X0 + (uint32_t)lane;
            const bool valid = X >= xa && X <= xb;
            resize_phase_horizontal(a, s, sums(t), valid ? a.cols[X - f.dx] : cb, valid, c);
        });
        wave_fence();                                         // (the next chunk's column sums overwrite these)
    }
}

template <class EachLane>
H263_HD void framed_resize_item(const FramedResizeArgs &fa, ResizeLds &s, uint32_t band, uint32_t seg, uint32_t pic, EachLane each)
{
    const ResizeArgs &a = fa.r;
    const FrameRect &f = fa.f;
    uint8_t *const pic_dst = a.dst[pic];
    if (!pic_dst) return;                                     // a stream with nothing to render: untouched
    const uint8_t *const pic_src = a.src + (size_t)pic * a.w * a.h * 4u;
    const uint32_t X0 = seg * 64u, X1 = (X0 + 64u < f.cw ? X0 + 64u : f.cw) - 1u;
    uint32_t xa, xb;
    const bool cols_in = frame_columns(f, a.ow, X0, X1, xa, xb);
    if (!cols_in && f.keep) return;
    const uint32_t Y0 = band * RESIZE_ROWS, Y1 = Y0 + RESIZE_ROWS < f.ch ? Y0 + RESIZE_ROWS : f.ch;
    const uint32_t half = a.d >> 1;
    for (uint32_t Y = Y0; Y < Y1; Y++) {
        const bool row_in = cols_in && Y >= f.dy && Y < f.dy + a.oh;
        if (!row_in && f.keep) continue;
        if (row_in) {
            each([&](int lane, ResizeLane &t) { t.acc[0] = t.acc[1] = t.acc[2] = 0; });
            framed_phases<ResizeLane>(a, f, s, pic_src, Y, X0, xa, xb, each, [](ResizeLane &t) -> ResizeLane & { return t; });
        }
        each([&](int lane, ResizeLane &t) {
            const uint32_t X = X0 + (uint32_t)lane;
            if (X > X1) return;
            const bool inside = row_in && X >= xa && X <= xb;
            if (!inside && f.keep) return;
            uint32_t px = f.pad;
            if (inside)
                px = resize_div(t.acc[0] + half, a.d, a.inv_d) | (resize_div(t.acc[1] + half, a.d, a.inv_d) << 8) |
                     (resize_div(t.acc[2] + half, a.d, a.inv_d) << 16);
            *reinterpret_cast<uint32_t *>(pic_dst + (size_t)Y * a.pitch + (size_t)X * 4u) = px | 0xff000000u;
        });
    }
}

}  // namespace h263mi
