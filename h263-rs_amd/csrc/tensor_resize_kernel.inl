// tensor_resize_kernel.inl -- k_tensor_resize: full-size RGBA -> the normalised planar 3 x H' x W' tensor of one stream, in
// binary32, binary16 or bfloat16 (h263mi_tensor_out, ABI 7).
//
// The contract (include/h263mi.h): with u (0..255) the channel value of the area average that k_rgba_resize stores,
//     v = fl32(fl32((float)u * scale[c]) + bias[c])            two roundings to nearest even, never fused, subnormals kept
// and for the 16-bit types v converted with round-to-nearest-even (overflow: +-inf, subnormal results kept).  Element (p, Y, X)
// of a picture lies p*stride_c + Y*stride_h + X elements behind its pointer; plane p holds colour p, or 2 - p (bgr).
//
// Phases 1 and 2 are k_rgba_resize's own (resize_kernel.inl: the same functions, the same launch shape -- one wave per workgroup,
// no barrier, a wave = 64 output columns x RESIZE_ROWS output rows, bands in XCD order).  Phase 3 is new: three u, converted,
// scaled, biased, then three planar stores.  For the 16-bit types neighbouring columns leave as one 32-bit store wherever the
// element's address is a multiple of 4: every lane hands its three binary32 values through LDS, the lane at the aligned address
// converts its own and its right neighbour's (v_cvt_pk_bf16_f32 for bfloat16) and stores both; an element that has no partner --
// the last column, the wave's last lane, the wave's first lane at an odd element address -- leaves as a 16-bit store.  So any base
// alignment, any stride_h and any W' are served, and the aligned case stores whole dwords.
//
// The multiply and the add stay two instructions whatever -ffp-contract the command line carries: the product passes through
// an empty asm statement, so the compiler cannot see a multiply to fuse into the add (a `#pragma clang fp contract(off)` is
// not enough: -ffp-contract=fast lets the gfx950 back end fuse on its own, and HIP's __fmul_rn is a plain product here).
// (g++, which builds the CPU checker, has no fused instruction to choose on its default target.)
//
// Written in the H263_HD style of the other kernels: tests/sim_tensor/ runs tensor_resize_item lane by lane under g++
// (ASan / UBSan); the host build converts to the 16-bit types with the integer code below, bit for bit what the device's
// conversion instructions give.
#pragma once

#include "resize_kernel.inl"

namespace h263mi {

constexpr uint32_t TENSOR_F32 = 0, TENSOR_F16 = 1, TENSOR_BF16 = 2;      // (H263MI_TENSOR_*)

struct TensorArgs {
    ResizeArgs r;                // src, dst (picture p's tensor at dst[p], nullptr = skip p), spans and sizes; pitch unused
    float scale[3], bias[3];     // per COLOUR R, G, B
    uint32_t dtype;              // TENSOR_*
    uint32_t bgr;                // plane p holds colour 2 - p
    uint64_t stride_c, stride_h; // in elements; one picture spans less than 2^32 bytes (h263mi_tensor_extent)
};

// the launch of k_tensor_resize (HOST): k_rgba_resize's shape
inline bool tensor_resize_plan(TensorArgs &a, LaunchDims &d)
{
    if (a.r.n_pictures > 65535 || a.dtype > TENSOR_BF16) return false;
    return resize_plan(a.r, d);
}

// what a lane keeps across the phases of one output row
struct TensorLane {
    ResizeLane sums;
    uint32_t v[3];               // the normalised values per colour, binary32 bits
};

H263_HD uint32_t tensor_bits_of(float f)
{
    uint32_t b;
    __builtin_memcpy(&b, &f, 4);
    return b;
}

// fl32(fl32(u * scale) + bias): never contracted into a fused multiply-add
H263_HD float tensor_value(uint32_t u, float scale, float bias)
{
    float m = (float)u * scale;
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(m));                                        // (no instruction: the product is opaque to the add below)
#endif
    return m + bias;
}

// binary32 bits -> bfloat16 bits, round to nearest even (never a NaN here: scale and bias are finite, so v is finite or +-inf)
H263_HD uint32_t tensor_bf16_bits(uint32_t b) { return (uint32_t)(((uint64_t)b + 0x7fffu + ((b >> 16) & 1u)) >> 16); }

// binary32 bits -> binary16 bits, round to nearest even, subnormal results kept, overflow to infinity
H263_HD uint32_t tensor_f16_bits_int(uint32_t b)
{
    const uint32_t sign = (b >> 16) & 0x8000u, a = b & 0x7fffffffu;
    if (a > 0x7f800000u) return sign | 0x7e00u;
    if (a >= 0x477ff000u) return sign | 0x7c00u;              // 65520 = halfway between 65504 and 2^16: ties to even, infinity
    if (a >= 0x38800000u) {                                   // 2^-14 and above: a normal binary16
        uint32_t r = a - 0x38000000u;                         // (exponent bias 127 -> 15)
        r += 0xfffu + ((r >> 13) & 1u);
        return sign | (r >> 13);
    }
    if (a < 0x33000000u) return sign;                         // below 2^-25: zero (2^-25 itself ties to even, zero, below)
    // a subnormal binary16: the significand in units of 2^-24
    const uint32_t e = a >> 23, m = (a & 0x7fffffu) | 0x800000u, shift = 126u - e;       // e = 102..112: shift = 24..14
    uint32_t q = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
    if (rem > half || (rem == half && (q & 1u))) q++;
    return sign | q;
}

H263_HD uint32_t tensor_f16_bits(uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    float f;
    __builtin_memcpy(&f, &b, 4);
    const _Float16 h = (_Float16)f;                           // v_cvt_f16_f32: the wave's rounding mode is nearest even
    uint16_t r;
    __builtin_memcpy(&r, &h, 2);
    return r;
#else
    return tensor_f16_bits_int(b);
#endif
}

// one value (binary32 bits) as a 16-bit element of `dtype`
H263_HD uint32_t tensor_cvt16(uint32_t dtype, uint32_t b) { return dtype == TENSOR_BF16 ? tensor_bf16_bits(b) : tensor_f16_bits(b); }

// two neighbouring values as one word: `lo` at the lower address
H263_HD uint32_t tensor_pack16(uint32_t dtype, uint32_t lo, uint32_t hi)
{
    if (dtype == TENSOR_BF16) {
#if defined(__HIP_DEVICE_COMPILE__)
        uint32_t r;
        asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
        return r;
#else
        return tensor_bf16_bits(lo) | (tensor_bf16_bits(hi) << 16);
#endif
    }
    return tensor_f16_bits(lo) | (tensor_f16_bits(hi) << 16);
}

// Phase 3, first half: round and divide as k_rgba_resize does, then normalise -- the lane's three values per colour
H263_HD void tensor_phase_value(const TensorArgs &a, TensorLane &t)
{
    const uint32_t half = a.r.d >> 1;
    for (int c = 0; c < 3; c++)
        t.v[c] = tensor_bits_of(tensor_value(resize_div(t.sums.acc[c] + half, a.r.d, a.r.inv_d), a.scale[c], a.bias[c]));
}

// the byte address of element (p, Y, X) of a picture
H263_HD uint8_t *tensor_at(const TensorArgs &a, uint8_t *pic_dst, uint32_t p, uint32_t Y, uint32_t X, uint32_t elt)
{
    return pic_dst + ((size_t)p * a.stride_c + (size_t)Y * a.stride_h + X) * elt;
}

// Phase 3 for binary32: three planar dword stores
H263_HD void tensor_phase_store32(const TensorArgs &a, const TensorLane &t, uint8_t *pic_dst, uint32_t X, uint32_t Y, bool valid)
{
    if (!valid) return;
    for (uint32_t p = 0; p < 3; p++) *reinterpret_cast<uint32_t *>(tensor_at(a, pic_dst, p, Y, X, 4)) = t.v[a.bgr ? 2u - p : p];
}

// Phase 3 for the 16-bit types, after every lane's values went into LDS (s.v[colour][lane]): the lane at a dword address stores
// its element and its right neighbour's as one word
H263_HD void tensor_phase_store16(const TensorArgs &a, const ResizeLds &s, const TensorLane &t, int lane, uint8_t *pic_dst, uint32_t X,
                                  uint32_t X1, uint32_t Y)
{
    if (X > X1) return;
    for (uint32_t p = 0; p < 3; p++) {
        const uint32_t c = a.bgr ? 2u - p : p;
        uint8_t *const at = tensor_at(a, pic_dst, p, Y, X, 2);
        if (((uintptr_t)at & 2u) == 0) {
            if (lane < 63 && X < X1) *reinterpret_cast<uint32_t *>(at) = tensor_pack16(a.dtype, t.v[c], s.v[c][lane + 1]);
            else *reinterpret_cast<uint16_t *>(at) = (uint16_t)tensor_cvt16(a.dtype, t.v[c]);
        } else if (lane == 0) {
            *reinterpret_cast<uint16_t *>(at) = (uint16_t)tensor_cvt16(a.dtype, t.v[c]);
        }
        // (every other element at an odd address left with the lane to its left)
    }
}

// One wave's work: the 64 output columns of segment `seg` in band `band` of picture `pic`, all three planes.  `each(f)` runs
// f(lane, lane_state) for the lanes this thread stands for: the one of its hardware lane on the GPU, all 64 in turn in the CPU
// checker.  Everything outside `each` is wave-uniform.
template <class EachLane>
H263_HD void tensor_resize_item(const TensorArgs &a, ResizeLds &s, uint32_t band, uint32_t seg, uint32_t pic, EachLane each)
{
    const ResizeArgs &r = a.r;
    uint8_t *const pic_dst = r.dst[pic];
    if (!pic_dst) return;                                     // a stream with nothing to render: untouched
    const uint8_t *const pic_src = r.src + (size_t)pic * r.d * 4u;
    const uint32_t X0 = seg * 64u, X1 = (X0 + 64u < r.ow ? X0 + 64u : r.ow) - 1u;
    const uint32_t c0 = r.cols[X0].first & ~3u, c_end = r.cols[X1].first + r.cols[X1].count;
    const uint32_t Y0 = band * RESIZE_ROWS, Y1 = Y0 + RESIZE_ROWS < r.oh ? Y0 + RESIZE_ROWS : r.oh;
    for (uint32_t Y = Y0; Y < Y1; Y++) {
        const ResizeSpan rs = r.rows[Y];
        each([&](int lane, TensorLane &t) { t.sums.acc[0] = t.sums.acc[1] = t.sums.acc[2] = 0; });
        for (uint32_t c = c0; c < c_end; c += RESIZE_CHUNK) {
            each([&](int lane, TensorLane &) { resize_phase_vertical(r, s, lane, pic_src, rs, c, c_end); });
            wave_fence();
            each([&](int lane, TensorLane &t) {
                const uint32_t X = X0 + (uint32_t)lane;
                const bool valid = X <= X1;
                resize_phase_horizontal(r, s, t.sums, valid ? r.cols[X] : r.cols[X1], valid, c);
            });
            wave_fence();                                     // (the next chunk's column sums, or the values below, overwrite these)
        }
        if (a.dtype == TENSOR_F32) {
            each([&](int lane, TensorLane &t) {
                tensor_phase_value(a, t);
                tensor_phase_store32(a, t, pic_dst, X0 + (uint32_t)lane, Y, X0 + (uint32_t)lane <= X1);
            });
        } else {
            each([&](int lane, TensorLane &t) {
                tensor_phase_value(a, t);
                for (int c = 0; c < 3; c++) s.v[c][lane] = t.v[c];
            });
            wave_fence();
            each([&](int lane, TensorLane &t) { tensor_phase_store16(a, s, t, lane, pic_dst, X0 + (uint32_t)lane, X1, Y); });
            wave_fence();                                     // (the next row's column sums overwrite the values)
        }
    }
}

// ---------------------------------------------------------------------------------------
// k_tensor_resize_framed: k_rgba_resize_framed (resize_kernel.inl: FrameRect, the meaning of t.r) ending in the tensor's stores.
// The pad colour is a `u` like any other: it is scaled, biased and converted by the same code, and for the 16-bit types it goes
// through the same LDS hand-off as the picture's values, so a pair that straddles the rectangle's edge still leaves as one
// 32-bit store.  With `keep` only the columns [wa, wb] of the rectangle may be written: a pair needs both elements in that
// range, the first of the range at an odd address leaves alone -- an element outside is never written, whatever the base
// alignment, stride_h, dx and dw are.
// ---------------------------------------------------------------------------------------
struct FramedTensorArgs {
    TensorArgs t;
    FrameRect f;
};

// the launch of k_tensor_resize_framed (HOST): k_rgba_resize_framed's shape
inline bool framed_tensor_plan(FramedTensorArgs &a, LaunchDims &d)
{
    if (a.t.r.n_pictures > 65535 || a.t.dtype > TENSOR_BF16) return false;
    return framed_plan(a.t.r, a.f, d);
}

// tensor_phase_store16 for the columns [wa, wb] of a row: the lane at a dword address stores its element and its right
// neighbour's as one word where the neighbour is in the range and in the wave
H263_HD void framed_phase_store16(const TensorArgs &a, const ResizeLds &s, const TensorLane &t, int lane, uint8_t *pic_dst, uint32_t X,
                                  uint32_t wa, uint32_t wb, uint32_t Y)
{
    if (X < wa || X > wb) return;
    for (uint32_t p = 0; p < 3; p++) {
        const uint32_t c = a.bgr ? 2u - p : p;
        uint8_t *const at = tensor_at(a, pic_dst, p, Y, X, 2);
        if (((uintptr_t)at & 2u) == 0) {
            if (lane < 63 && X < wb) *reinterpret_cast<uint32_t *>(at) = tensor_pack16(a.dtype, t.v[c], s.v[c][lane + 1]);
            else *reinterpret_cast<uint16_t *>(at) = (uint16_t)tensor_cvt16(a.dtype, t.v[c]);
        } else if (lane == 0 || X == wa) {
            *reinterpret_cast<uint16_t *>(at) = (uint16_t)tensor_cvt16(a.dtype, t.v[c]);
        }
        // (every other element at an odd address left with the lane to its left: that one is in the range and in the wave)
    }
}

template <class EachLane>
H263_HD void framed_tensor_item(const FramedTensorArgs &fa, ResizeLds &s, uint32_t band, uint32_t seg, uint32_t pic, EachLane each)
{
    const TensorArgs &a = fa.t;
    const ResizeArgs &r = a.r;
    const FrameRect &f = fa.f;
    uint8_t *const pic_dst = r.dst[pic];
    if (!pic_dst) return;                                     // a stream with nothing to render: untouched
    const uint8_t *const pic_src = r.src + (size_t)pic * r.w * r.h * 4u;
    const uint32_t X0 = seg * 64u, X1 = (X0 + 64u < f.cw ? X0 + 64u : f.cw) - 1u;
    uint32_t xa, xb;
    const bool cols_in = frame_columns(f, r.ow, X0, X1, xa, xb);
    if (!cols_in && f.keep) return;
    const uint32_t Y0 = band * RESIZE_ROWS, Y1 = Y0 + RESIZE_ROWS < f.ch ? Y0 + RESIZE_ROWS : f.ch;
    for (uint32_t Y = Y0; Y < Y1; Y++) {
        const bool row_in = cols_in && Y >= f.dy && Y < f.dy + r.oh;
        if (!row_in && f.keep) continue;
        if (row_in) {
            each([&](int lane, TensorLane &t) { t.sums.acc[0] = t.sums.acc[1] = t.sums.acc[2] = 0; });
            framed_phases<TensorLane>(r, f, s, pic_src, Y, X0, xa, xb, each, [](TensorLane &t) -> ResizeLane & { return t.sums; });
        }
        // the columns this row writes
        const uint32_t wa = f.keep ? xa : X0, wb = f.keep ? xb : X1;
        auto value = [&](int lane, TensorLane &t) {
            const uint32_t X = X0 + (uint32_t)lane;
            if (row_in && X >= xa && X <= xb) {
                tensor_phase_value(a, t);
            } else {
                for (int c = 0; c < 3; c++) t.v[c] = tensor_bits_of(tensor_value((f.pad >> (8 * c)) & 0xffu, a.scale[c], a.bias[c]));
            }
        };
        if (a.dtype == TENSOR_F32) {
            each([&](int lane, TensorLane &t) {
                const uint32_t X = X0 + (uint32_t)lane;
                value(lane, t);
                tensor_phase_store32(a, t, pic_dst, X, Y, X >= wa && X <= wb);
            });
        } else {
            each([&](int lane, TensorLane &t) {
                value(lane, t);
                for (int c = 0; c < 3; c++) s.v[c][lane] = t.v[c];
            });
            wave_fence();
            each([&](int lane, TensorLane &t) { framed_phase_store16(a, s, t, lane, pic_dst, X0 + (uint32_t)lane, wa, wb, Y); });
            wave_fence();                                     // (the next row's column sums overwrite the values)
        }
    }
}

}  // namespace h263mi
