// roi_kernel.inl -- k_roi_tensor: a DEVICE table of regions of interest over full-size RGBA -> one normalised planar tensor per
// region, K x 3 x H' x W' in binary32, binary16 or bfloat16 (h263mi_roi, h263mi_roi_tensor_on; ABI 7).
//
// The contract (include/h263mi.h): element (k, p, Y, X) is what k_tensor_resize_framed gives for H263MI_FRAME_WINDOW with the
// source rectangle (x, y, w, h) of region k and the destination (0, 0, W', H'): the area average with divisor w*h, one rounding
// half up, then fl32(fl32(u * scale[c]) + bias[c]), converted as h263mi_tensor_out documents.  A region that is not valid
// (reserved set, picture >= n_pictures, w or h 0, x + w > width, y + h > height) reads nothing of the pictures and writes no
// element; its status word becomes 1, a valid region's 0.
//
// Phases 1, 2 and 3 are k_tensor_resize's own (resize_kernel.inl, tensor_resize_kernel.inl: the same functions, the same launch
// shape with the region in the place of the picture -- one wave per workgroup, no barrier, a wave = 64 output columns x
// RESIZE_ROWS output rows, bands in XCD order).  What is new is the head of a wave's work: it reads its 16-byte record (wave-
// uniform), validates it, and makes the ResizeSpans that the host makes for the other kernels -- the row spans of its rows
// (uniform), each lane's column span -- without a division instruction:
//   * by W' and H', known on the host: roi_div with a host-made reciprocal;
//   * by d = w*h, known here only: resize_div with inv_d made by v_rcp_f32 (bound below).
// What bounds every access: a valid region lies inside picture `picture` < n_pictures, its spans lie inside the region (they are
// resize_spans' own, offset by x / y), phase 1 reads whole groups of 4 columns of the picture's row that never pass the row's end
// (resize_phase_vertical), and phase 3 writes columns < W' of rows < H' of tensor k < n_rois.  The host has checked that the
// n_pictures pictures and the n_rois tensors lie inside the two buffers.
//
// Written in the H263_HD style of the other kernels: tests/sim_roi/ runs roi_tensor_item lane by lane under g++ (ASan / UBSan).
#pragma once

#include "tensor_resize_kernel.inl"

namespace h263mi {

// h263mi_roi as the device reads it: four words
struct RoiRecord {
    uint32_t picture;
    uint32_t xy;                 // x | y << 16
    uint32_t wh;                 // w | h << 16
    uint32_t reserved;
};

struct RoiArgs {
    TensorArgs t;                // t.r: src, w, h (the pictures), ow, oh (W', H'), n_pictures, bands, chunk; dst, cols, rows, pitch, d
                                 // and inv_d are not used (a wave makes its own); scale, bias, dtype, bgr, stride_c, stride_h
    const RoiRecord *rois;       // DEVICE, n_rois records: read by the waves only
    uint8_t *dst;                // region k's tensor at dst + k * stride_n elements
    uint64_t stride_n;           // in elements
    uint32_t *status;            // DEVICE, n_rois words, or nullptr
    uint32_t n_rois;
    float inv_ow, inv_oh;        // fl(1 / W'), fl(1 / H'): made on the host with a division
};

// the launch of k_roi_tensor (HOST): k_tensor_resize's shape with the region in the place of the picture
inline bool roi_plan(RoiArgs &a, LaunchDims &d)
{
    ResizeArgs &r = a.t.r;
    if (a.n_rois > 65535 || a.t.dtype > TENSOR_BF16 || !r.ow || !r.oh || r.ow > 65535 || r.oh > 65535 || !r.w || !r.h || r.w > 65535 ||
        r.h > 65535 || (uint64_t)r.w * r.h >= (1ull << 30) || !r.n_pictures || !r.src || !a.rois || !a.dst)
        return false;
    d = band_grid(r.oh, RESIZE_ROWS, a.n_rois, (r.ow + 63) / 64, r.bands, r.chunk);
    return true;
}

// what a lane keeps across the rows of a wave
struct RoiLane {
    TensorLane t;
    ResizeSpan cs;               // the span of the lane's output column
};

// n div d for 1 <= d <= 65535 and n < 65535 * d -- exact, without an integer division instruction; inv = fl(1 / d).
//
// Where it is used n is X * size or (X + 1) * size - 1 with X < d = W' (H') and size <= 65535, so n < 65535 * d <= 65535^2 < 2^32
// and x = n / d < 65535.  The estimate is f = fl(fl(n) * inv): the conversion of n (32 bits into 24, to nearest), the division
// behind inv (d < 2^16 converts exactly) and the product are one rounding of at most 2^-24 relative each, so f = x * (1 + e) with
// |e| <= 3 * 2^-24 + 3 * 2^-48 + 2^-72 < 2^-22 and |f - x| < 65535 * 2^-22 < 2^-6.  Hence q0 = trunc(f) differs from q = floor(x)
// by at most one (f >= 0, and f < 65535 + 2^-6 gives q0 <= 65535: q0 * d < 2^32), and r = n - q0 * d lies in [-d, 2d), which
// 32 signed bits hold: r < 0 -> q0 - 1, r >= d -> q0 + 1.  tests/sim_roi compares the spans made with it against resize_spans for
// every (size, out) of 1..400 x 1..300 and with 65535 on either side.
H263_HD uint32_t roi_div(uint32_t n, uint32_t d, float inv)
{
    uint32_t q = (uint32_t)((float)n * inv);
    const int32_t r = (int32_t)(n - q * d);
    if (r < 0) q--;
    else if (r >= (int32_t)d) q++;
    return q;
}

// resize_spans' entry X of (size, out), `first` offset by `origin`: every product is at most 65535^2 < 2^32 (X < out)
H263_HD ResizeSpan roi_span(uint32_t X, uint32_t size, uint32_t out, float inv_out, uint32_t origin)
{
    const uint32_t lo = X * size, hi = lo + size;
    const uint32_t first = roi_div(lo, out, inv_out), last = roi_div(hi - 1u, out, inv_out);
    const uint32_t first_end = (first + 1u) * out, last_begin = last * out;
    ResizeSpan sp;
    sp.first = origin + first;
    sp.count = last - first + 1u;
    sp.w_first = (hi < first_end ? hi : first_end) - lo;
    sp.w_last = hi - (lo > last_begin ? lo : last_begin);
    return sp;
}

// The reciprocal of d = w*h (1 <= d < 2^30) for resize_div, made on the device.
//
// resize_div's bound (resize_kernel.inl) redone for it: with n = num + floor(d/2) < 2^38 and x = n / d <= 255.5 the estimate is
// f = fl(fl(n) * inv_d).  fl(n) is off by at most 2^-23 relative (a truncating conversion), fl(d) by 2^-24 (d has up to 30
// bits), v_rcp_f32 of it by 1 ulp = at most 2^-23 relative, the product by 2^-24: f = x * (1 + e) with
// |e| <= 2^-23 + 2^-24 + 2^-23 + 2^-24 + (products of these, < 2^-44) < 2^-21, so |f - x| <= 255.5 * 2^-21 < 2^-12 -- the bound
// that resize_div's proof needs, with the same conclusion: q0 = trunc(f) is off by at most one, q0 <= 256, and the one correction
// makes it exact.  The host's 1.0f / d meets the same bound (its division is one rounding of 2^-24), so the CPU checker and the
// device may differ in inv_d's last bit and never in a quotient.  tests/sim_roi checks n = q*d - 1, q*d, q*d + d/2 for every q of
// 0..255 at the largest d with inv_d = fl(1/d) and both its neighbours.
// (v_rcp_f32, not 1.0f / d: the IEEE division expands to a sequence with fused multiply-adds, which this library's kernels do
// not hold -- tests/test_abi.py.)
H263_HD float roi_inv_d(uint32_t d)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf((float)d);
#else
    return 1.0f / (float)d;
#endif
}

// a record's fields, and whether they name a rectangle of one of the pictures (the sums in 32 bits: x + w <= 131070)
struct RoiRect {
    uint32_t picture, x, y, w, h;
    bool valid;
};

H263_HD RoiRect roi_rect(const RoiRecord &q, uint32_t n_pictures, uint32_t width, uint32_t height)
{
    RoiRect r;
    r.picture = q.picture;
    r.x = q.xy & 0xffffu, r.y = q.xy >> 16;
    r.w = q.wh & 0xffffu, r.h = q.wh >> 16;
    r.valid = q.reserved == 0 && q.picture < n_pictures && r.w >= 1u && r.h >= 1u && r.x + r.w <= width && r.y + r.h <= height;
    return r;
}

// One wave's work: the 64 output columns of segment `seg` in band `band` of region `k`, all three planes.  `each(f)` runs
// f(lane, lane_state) for the lanes this thread stands for: the one of its hardware lane on the GPU, all 64 in turn in the CPU
// checker.  Everything outside `each` is wave-uniform.
template <class EachLane>
H263_HD void roi_tensor_item(const RoiArgs &ra, ResizeLds &s, uint32_t band, uint32_t seg, uint32_t k, EachLane each)
{
    const RoiRect q = roi_rect(ra.rois[k], ra.t.r.n_pictures, ra.t.r.w, ra.t.r.h);
    if (band == 0 && seg == 0 && ra.status)
        each([&](int lane, RoiLane &) {
            if (lane == 0) ra.status[k] = q.valid ? 0u : 1u;
        });
    if (!q.valid) return;                                     // nothing of the pictures is read, no element is written
    // the resize inside the region, as FramedResizeArgs::r describes it: d = sw*sh, the spans offset by x / y, the row stride the picture's
    TensorArgs a = ra.t;
    ResizeArgs &r = a.r;
    r.d = q.w * q.h;                                          // (<= width * height < 2^30)
    r.inv_d = roi_inv_d(r.d);
    const uint32_t elt = a.dtype == TENSOR_F32 ? 4u : 2u;
    uint8_t *const pic_dst = ra.dst + (size_t)k * ra.stride_n * elt;
    const uint8_t *const pic_src = r.src + (size_t)q.picture * r.w * r.h * 4u;
    const uint32_t X0 = seg * 64u, X1 = (X0 + 64u < r.ow ? X0 + 64u : r.ow) - 1u;
    const ResizeSpan ca = roi_span(X0, q.w, r.ow, ra.inv_ow, q.x), cb = roi_span(X1, q.w, r.ow, ra.inv_ow, q.x);
    const uint32_t c0 = ca.first & ~3u, c_end = cb.first + cb.count;
    each([&](int lane, RoiLane &t) {
        const uint32_t X = X0 + (uint32_t)lane;
        t.cs = roi_span(X <= X1 ? X : X1, q.w, r.ow, ra.inv_ow, q.x);
    });
    const uint32_t Y0 = band * RESIZE_ROWS, Y1 = Y0 + RESIZE_ROWS < r.oh ? Y0 + RESIZE_ROWS : r.oh;
    for (uint32_t Y = Y0; Y < Y1; Y++) {
        const ResizeSpan rs = roi_span(Y, q.h, r.oh, ra.inv_oh, q.y);
        each([&](int lane, RoiLane &t) { t.t.sums.acc[0] = t.t.sums.acc[1] = t.t.sums.acc[2] = 0; });
        for (uint32_t c = c0; c < c_end; c += RESIZE_CHUNK) {
            each([&](int lane, RoiLane &) { resize_phase_vertical(r, s, lane, pic_src, rs, c, c_end); });
            wave_fence();
            each([&](int lane, RoiLane &t) { resize_phase_horizontal(r, s, t.t.sums, t.cs, X0 + (uint32_t)lane <= X1, c); });
            wave_fence();                                     // (the next chunk's column sums, or the values below, overwrite these)
        }
        if (a.dtype == TENSOR_F32) {
            each([&](int lane, RoiLane &t) {
                tensor_phase_value(a, t.t);
                tensor_phase_store32(a, t.t, pic_dst, X0 + (uint32_t)lane, Y, X0 + (uint32_t)lane <= X1);
            });
        } else {
            each([&](int lane, RoiLane &t) {
                tensor_phase_value(a, t.t);
                for (int c = 0; c < 3; c++) s.v[c][lane] = t.t.v[c];
            });
            wave_fence();
            each([&](int lane, RoiLane &t) { tensor_phase_store16(a, s, t.t, lane, pic_dst, X0 + (uint32_t)lane, X1, Y); });
            wave_fence();                                     // (the next row's column sums overwrite the values)
        }
    }
}

}  // namespace h263mi
