// output_shape.h -- the SHAPE a rendering writes its output in: the RGBA layouts and resizes (h263mi_rgba_layout,
// h263mi_rgba_resize), the float tensor that a resize may end in (h263mi_tensor_out) and the plane layouts and resizes (h263mi_yuv_layout, h263mi_yuv_resize).  A caller's placement is
// validated here (the *_extent entry points), turned into what the kernels are told, and given the device memory it needs: the
// plane offsets of a YUV layout, the scratch and the span tables of a resize.  Nothing here knows a frame store: a batch holds
// one RgbaLayout and one YuvLayout (batch.h) and hands them to its renderings.
#pragma once

#include <memory>
#include <vector>

#include "host_common.h"

namespace h263mi {

// One allocation of device memory and its owner: freed on the device it was made on.  Shared (shared_ptr) between a batch's
// shape and the pending rendering that was requested under it, so that switching the shape while a pipelined rendering waits
// frees nothing that rendering still needs.
struct DeviceBlock {
    int device = 0;
    void *p = nullptr;
    uint64_t bytes = 0;
    DeviceBlock() = default;
    DeviceBlock(const DeviceBlock &) = delete;
    DeviceBlock &operator=(const DeviceBlock &) = delete;
    ~DeviceBlock() { release(); }
    void release();
    // `n` bytes on `dev`, the current device (the caller holds a DeviceGuard); with `from`: filled from that host memory
    int make(int dev, uint64_t n, const void *from = nullptr);
    // a scratch that only grows: room for `n` bytes (what it held is not kept)
    int reserve(int dev, uint64_t n);
    template <typename T>
    T *as() const { return static_cast<T *>(p); }
};

// What a resize kernel reads (k_rgba_resize, k_plane_resize): the full-size pictures that the rendering kernels write for it --
// RGBA, n * w*h*4 bytes, or planes, tightly packed I420 per stream, n * (w*h + 2*cw*ch) bytes -- and the spans of its geometry:
// W' column spans then H' row spans, for planes followed by the cW' and cH' spans of the chroma planes.
// Under a filter (h263mi_filter: k_rgba_filter, k_tensor_filter, k_plane_filter) `spans` holds the tap tables instead
// (filter_taps.h: filter_table; for planes the luma table, then the chroma table).
struct ResizeScratch {
    DeviceBlock pixels, spans;             // (two allocations: resize_scratch_bytes counts both)
};

// What the kernels are told of an RGBA output layout (PostArgs::rgba_scale, rgba_pitch; pitch 0 = the default layout)
struct OutLayout {
    uint32_t scale = 0, pitch = 0;
};

// The output shape of the RGBA (h263mi_batch_set_rgba_layout, _set_rgba_resize).  `kernel`: what the kernels are told (pitch 0:
// the default kernels); `offsets` (empty = s * H' * pitch): where stream s's picture starts in the caller's buffer -- handed to
// the kernels as per-stream pointers.
struct RgbaLayout {
    OutLayout kernel;
    std::vector<uint64_t> offsets;
    uint64_t bytes = 0;                    // what d_rgba must hold (h263mi_rgba_layout_extent)
    bool placed() const { return kernel.pitch != 0; }
    // a resize that is not one of the layouts (scratch != nullptr): the rendering kernels write the full-size pictures into
    // the scratch with the default `kernel`, then k_rgba_resize writes W' x H' at `offsets` (all of them filled in)
    struct Resize {
        std::shared_ptr<ResizeScratch> scratch;
        uint32_t ow = 0, oh = 0, pitch = 0;
        // ... or the resize ends in a tensor (h263mi_batch_set_tensor_output: k_tensor_resize instead of k_rgba_resize; `offsets`
        // are then the BYTE offsets of the streams' tensors, pitch is not used): the whole description, copied
        struct Tensor {
            bool on = false;
            uint32_t dtype = 0, bgr = 0, elt = 4;      // (elt: bytes per element)
            float scale[3] = {1, 1, 1}, bias[3] = {0, 0, 0};
            uint64_t stride_c = 0, stride_h = 0;       // in elements, defaults spelled out
        } tensor;
        // ... and it may be framed (h263mi_framing that is not the unframed shape: k_rgba_resize_framed / k_tensor_resize_framed):
        // the resolved rectangles -- the scratch's span tables are then those of sw -> dw and sh -> dh, offset by sx / sy -- the
        // pad colour and keep_outside, copied
        struct Framed {
            bool on = false;
            h263mi_framing_rects rc{};
            uint32_t pad = 0;                          // R | G << 8 | B << 16
            bool keep = false;
        } framed;
        // ... or resampled with Pillow's bilinear or bicubic filter (h263mi_filter other than AREA: k_rgba_filter / k_tensor_filter
        // in the place of all four kernels above).  framed.rc is then always filled in (an unframed shape: the whole picture onto
        // the whole output), the scratch holds the tap tables of sw -> dw and sh -> dh, ksx / ksy entries per position
        struct Filter {
            bool on = false;
            uint32_t kind = 0, ksx = 0, ksy = 0;
        } filter;
        bool on() const { return scratch != nullptr; }
    } resize;
    // what a pointer into the caller's buffer must be a multiple of (a tensor: its element size)
    uint32_t base_align() const { return resize.on() && resize.tensor.on ? resize.tensor.elt : 1u; }
};

// The shape of the deblocked planes in d_deblocked (h263mi_batch_set_yuv_layout).  format 0: none -- tightly packed I420
// written by the default kernels.  Else the YUV instantiations write the planes (kernels.h: launch_post_yuv,
// launch_frame_yuv), and RGBA asked for in the same call is rendered by a launch of its own.
// Or the planes are RESIZED (h263mi_batch_set_yuv_resize; then format stays 0): the default kernels write the full-size
// planes into the resize's scratch and k_plane_resize follows them on the same stream.  A layout or a resize, never both.
struct YuvLayout {
    uint32_t format = 0;                   // 0, YUV_OUT_I420, YUV_OUT_NV12
    uint32_t pitch_y = 0, pitch_c = 0;
    bool wide = false;                     // pitches and offsets are all multiples of 4: the wide-store path
    std::shared_ptr<DeviceBlock> offsets;  // DEVICE: 3 per stream (Y, Cb or CbCr, Cr), uploaded once when the layout is set
    uint64_t bytes = 0;                    // what d_deblocked must hold (h263mi_yuv_layout_extent)
    bool on() const { return format != 0; }
    // what the kernels are told for planes at d_planes
    YuvOut out(const uint8_t *d_planes) const
    {
        YuvOut o{};
        o.format = format;
        o.wide = (wide && ((uintptr_t)d_planes & 3u) == 0) ? 1u : 0u;
        o.pitch_y = pitch_y;
        o.pitch_c = pitch_c;
        o.offsets = offsets ? offsets->as<uint64_t>() : nullptr;
        return o;
    }
    // a resize that is not the full-size layout (scratch != nullptr): W' x H' planes in `format` at `offsets` of d_deblocked
    struct Resize {
        std::shared_ptr<ResizeScratch> scratch;
        uint32_t format = 0;               // YUV_OUT_I420, YUV_OUT_NV12
        uint32_t ow = 0, oh = 0, pitch_y = 0, pitch_c = 0;
        bool wide = false;                 // pitches and offsets are all multiples of 4
        std::vector<uint64_t> offsets;     // 3 per stream: Y, Cb or CbCr, Cr
        // ... resampled with Pillow's bilinear or bicubic filter (h263mi_batch_set_yuv_resize_filtered, a kind other than AREA:
        // k_plane_filter in the place of k_plane_resize).  The scratch's `spans` then holds the luma and the chroma tap table
        // back to back (filter_taps.h: filter_table), ks* entries per position of each axis
        struct Filter {
            bool on = false;
            uint32_t kind = 0, ksx_y = 0, ksy_y = 0, ksx_c = 0, ksy_c = 0;
        } filter;
        bool on() const { return scratch != nullptr; }
    } resize;
    bool shaped() const { return on() || resize.on(); }      // (then `bytes` is what d_deblocked must hold)
};

// ---- what a caller's placement comes to (pure host functions: the *_extent entry points)
// h263mi_rgba_layout_extent; out_kernel (may be null): what the kernels are told (pitch 0 = the default layout)
int rgba_layout_extent(uint32_t n_streams, uint32_t w, uint32_t h, const h263mi_rgba_layout *layout, uint32_t *out_w,
                       uint32_t *out_h, uint64_t *bytes, OutLayout *out_kernel = nullptr);
// h263mi_yuv_layout_extent.  shape (may be null): format / pitches / wide / bytes filled in (no device memory);
// offsets (may be null): the 3 * n_streams plane offsets the kernels take (default placement spelled out)
int yuv_layout_extent(uint32_t n_streams, uint32_t w, uint32_t h, const h263mi_yuv_layout *layout, uint64_t *bytes,
                      YuvLayout *shape = nullptr, std::vector<uint64_t> *offsets = nullptr);
// A resize is placed as a layout of the W' x H' picture is: that layout (full size for RGBA: scale_log2 0)
h263mi_rgba_layout layout_of(const h263mi_rgba_resize &r);
h263mi_yuv_layout layout_of(const h263mi_yuv_resize &r);
// h263mi_rgba_resize_extent for n streams
int rgba_resize_extent(uint32_t n_streams, const h263mi_rgba_resize *r, uint64_t *bytes);
// h263mi_yuv_resize_extent; shape / offsets as yuv_layout_extent (of the W' x H' picture)
int yuv_resize_extent(uint32_t n_streams, const h263mi_yuv_resize *r, uint64_t *bytes, YuvLayout *shape = nullptr,
                      std::vector<uint64_t> *offsets = nullptr);
// h263mi_tensor_extent for n streams.  out (may be null): dtype, order, scale, bias and the strides with their defaults spelled
// out; stride_n (may be null): the streams' distance in elements
int tensor_extent(uint32_t n_streams, const h263mi_tensor_out *t, uint64_t *bytes, RgbaLayout::Resize::Tensor *out = nullptr,
                  uint64_t *stride_n = nullptr);
// h263mi_framing_resolve (f NULL: STRETCH); *whole (may be null): source whole and destination whole -- the unframed shape
int framing_resolve(uint32_t w, uint32_t h, uint32_t ow, uint32_t oh, const h263mi_framing *f, h263mi_framing_rects *out, bool *whole = nullptr);
// device memory a tensor output of `slots` pictures of w x h holds: always a scratch, whatever W' x H' (f: a framing that
// resolves for w x h -- its span tables are those of the destination rectangle)
// (flt: a filter that filter_kind accepts -- other than AREA the tap tables take the place of the span tables)
uint64_t tensor_scratch_bytes(uint32_t w, uint32_t h, uint32_t slots, const h263mi_tensor_out &t, const h263mi_framing *f = nullptr,
                              const h263mi_filter *flt = nullptr);
// the validation of an h263mi_filter (NULL: AREA); *kind (may be null): H263MI_FILTER_*
int filter_kind(const h263mi_filter *flt, uint32_t *kind = nullptr);
// the layout that a resize of a w x h picture is by definition (full size, or 1/2 or 1/4 of sizes that 2 or 4 divide), into
// *lay (offsets and pitch copied); false: none, the resize needs k_rgba_resize
bool resize_as_layout(uint32_t w, uint32_t h, const h263mi_rgba_resize &r, h263mi_rgba_layout *lay);
// device memory a resize of `slots` pictures of w x h holds (0: it is a layout)
uint64_t resize_scratch_bytes(uint32_t w, uint32_t h, uint32_t slots, const h263mi_rgba_resize &r, const h263mi_framing *f = nullptr,
                              const h263mi_filter *flt = nullptr);

// ---- the shapes, with the device memory they need, for n streams of w x h on `device`
// h263mi_batch_set_rgba_layout's (NULL: the default); no device memory
int make_rgba_layout_shape(uint32_t n, uint32_t w, uint32_t h, const h263mi_rgba_layout *layout, RgbaLayout &out);
// the RGBA shape `r` (NULL: the default): the layout it is by definition, or the resize with a new scratch
// f (h263mi_framing, NULL: none): a framing that resolves to the whole source and the whole destination is the unframed shape;
// every other one is the resize with a scratch, followed by k_rgba_resize_framed
// flt (h263mi_filter, NULL or AREA: none): always the resize with a scratch -- the full-size pictures and the tap tables --,
// followed by k_rgba_filter, whatever the sizes and the framing are
int make_output_shape(int device, uint32_t n, uint32_t w, uint32_t h, const h263mi_rgba_resize *r, RgbaLayout &out,
                      const h263mi_framing *f = nullptr, const h263mi_filter *flt = nullptr);
// the tensor shape `t` (NULL: the default): always the resize with a new scratch -- W' = w, H' = h too, where the area average is
// the identity -- followed by k_tensor_resize
// (f as make_output_shape: k_tensor_resize_framed)
// (flt as make_output_shape: k_tensor_filter)
int make_tensor_shape(int device, uint32_t n, uint32_t w, uint32_t h, const h263mi_tensor_out *t, RgbaLayout &out,
                      const h263mi_framing *f = nullptr, const h263mi_filter *flt = nullptr);
// the layout (NULL: none, format 0), its offsets uploaded
int make_yuv_shape(int device, uint32_t n, uint32_t w, uint32_t h, const h263mi_yuv_layout *layout, YuvLayout &out);
// the YUV shape `r` (NULL: none): the full-size layout it is by definition when W' = w and H' = h, else the resize with a new
// scratch
// flt (h263mi_filter, NULL or AREA: none): the resize with a scratch whose `spans` holds the four tap tables, followed by
// k_plane_filter; W' = w and H' = h stays the full-size layout under any filter
int make_yuv_resize_shape(int device, uint32_t n, uint32_t w, uint32_t h, const h263mi_yuv_resize *r, YuvLayout &out,
                          const h263mi_filter *flt = nullptr);

}  // namespace h263mi
