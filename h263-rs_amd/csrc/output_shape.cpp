// output_shape.cpp -- output shapes (output_shape.h): the placement rules of include/h263mi.h, what the kernels are told of a
// placement, and the device memory a shape needs.
#include "output_shape.h"

#include "filter_taps.h"

#include <algorithm>
#include <cmath>
#include <new>

namespace h263mi {

void DeviceBlock::release()
{
    if (!p) return;
    DeviceGuard g(device);
    (void)hipFree(p);
    p = nullptr;
    bytes = 0;
}

int DeviceBlock::make(int dev, uint64_t n, const void *from)
{
    device = dev;
    HIP_TRY(hipMalloc(&p, n));
    bytes = n;
    if (from) HIP_TRY(hipMemcpy(p, from, n, hipMemcpyHostToDevice));
    return H263MI_OK;
}

int DeviceBlock::reserve(int dev, uint64_t n)
{
    if (n <= bytes) return H263MI_OK;
    release();
    return make(dev, n);
}

// =========================================================================================
// placement
// =========================================================================================
// One plane of a placed output (an RGBA picture is the one plane of its stream): `rows` rows of `row` bytes, `pitch` bytes
// apart, at byte `offset` of the caller's buffer -- a rectangle on the grid of its pitch: rows [offset / pitch, + rows), byte
// columns [offset % pitch, + row).
struct PlaneRect {
    uint64_t pitch, row, rows, offset, align;
    bool chroma;                           // on the grid of the chroma pitch
    uint64_t span() const { return (rows - 1) * pitch + row; }       // bytes from the plane's first byte to behind its last
    uint64_t r0() const { return offset / pitch; }
    uint64_t c0() const { return offset % pitch; }
};

// what holds of a plane wherever it lies: its rows fit the pitch, and lane offsets are 32-bit
static bool plane_fits(uint64_t pitch, uint64_t row, uint64_t rows)
{
    if (pitch < row || (rows > 1 && pitch >= (1ull << 32))) return false;
    return (rows - 1) * pitch + row < (1ull << 32);
}
// what the kernels are told of a pitch (one row: the pitch is never used)
static uint32_t kernel_pitch(uint64_t pitch, uint64_t row, uint64_t rows) { return (uint32_t)(rows > 1 ? pitch : row); }

// The placement check: every plane aligned, inside the rows of its grid and inside 64 bits; no two planes of a grid
// sharing a byte; and, where the luma and the chroma grid differ, no luma plane's byte span meeting a chroma plane's.
// *extent: the bytes the buffer must hold.
static int planes_extent(std::vector<PlaneRect> planes, uint64_t *extent)
{
    uint64_t total = 0;
    bool one_grid = true;
    for (const PlaneRect &p : planes) {
        if (p.offset % p.align || p.c0() + p.row > p.pitch || p.offset > UINT64_MAX - p.span()) return H263MI_ERR_INVALID_ARGUMENT;
        total = std::max(total, p.offset + p.span());
        one_grid = one_grid && p.pitch == planes[0].pitch;
    }
    // within a grid (one grid for all planes: the rectangle test decides between luma and chroma too)
    std::sort(planes.begin(), planes.end(), [](const PlaneRect &x, const PlaneRect &y) { return x.r0() < y.r0() || (x.r0() == y.r0() && x.c0() < y.c0()); });
    for (size_t i = 0; i < planes.size(); i++)
        for (size_t j = i + 1; j < planes.size() && planes[j].r0() < planes[i].r0() + planes[i].rows; j++) {      // (sorted by first row: later ones start lower)
            const PlaneRect &a = planes[i], &b = planes[j];
            if ((one_grid || a.chroma == b.chroma) && b.c0() < a.c0() + a.row && a.c0() < b.c0() + b.row) return H263MI_ERR_INVALID_ARGUMENT;
        }
    if (!one_grid) {
        std::sort(planes.begin(), planes.end(), [](const PlaneRect &x, const PlaneRect &y) { return x.offset < y.offset; });
        uint64_t end_luma = 0, end_chroma = 0;
        for (const PlaneRect &p : planes) {
            if (p.offset < (p.chroma ? end_luma : end_chroma)) return H263MI_ERR_INVALID_ARGUMENT;
            uint64_t &e = p.chroma ? end_chroma : end_luma;
            e = std::max(e, p.offset + p.span());
        }
    }
    *extent = total;
    return H263MI_OK;
}

int rgba_layout_extent(uint32_t n_streams, uint32_t w, uint32_t h, const h263mi_rgba_layout *lay, uint32_t *out_w, uint32_t *out_h,
                       uint64_t *bytes, OutLayout *out_kernel)
{
    if (!n_streams || !w || !h) return H263MI_ERR_INVALID_ARGUMENT;
    const uint32_t scale = lay ? lay->scale_log2 : 0u;
    if (scale > 2) return H263MI_ERR_INVALID_ARGUMENT;
    if (lay)
        for (uint8_t r : lay->reserved)
            if (r) return H263MI_ERR_INVALID_ARGUMENT;
    const uint32_t ow = (w + (1u << scale) - 1) >> scale, oh = (h + (1u << scale) - 1) >> scale;
    const uint64_t row = 4ull * ow, pitch = (lay && lay->row_pitch) ? lay->row_pitch : row;
    if (pitch % 4 || !plane_fits(pitch, row, oh)) return H263MI_ERR_INVALID_ARGUMENT;
    uint64_t total = 0;
    const uint64_t *off = lay ? lay->offsets : nullptr;
    if (!off) {
        const unsigned __int128 t = (unsigned __int128)(n_streams - 1) * oh * pitch + (uint64_t)(oh - 1) * pitch + row;
        if (t > UINT64_MAX) return H263MI_ERR_INVALID_ARGUMENT;
        total = (uint64_t)t;
    } else {
        std::vector<PlaneRect> planes(n_streams);
        for (uint32_t i = 0; i < n_streams; i++) planes[i] = PlaneRect{pitch, row, oh, off[i], 4, false};
        RC_TRY(planes_extent(std::move(planes), &total));
    }
    if (out_w) *out_w = ow;
    if (out_h) *out_h = oh;
    if (bytes) *bytes = total;
    if (out_kernel) {
        // the default layout (full size, tight rows, pictures back to back) keeps the default kernels
        const bool dflt = scale == 0 && pitch == row && !off;
        out_kernel->scale = dflt ? 0u : scale;
        out_kernel->pitch = dflt ? 0u : kernel_pitch(pitch, row, oh);
    }
    return H263MI_OK;
}

// h263mi_yuv_layout_extent (include/h263mi.h has the rules)
int yuv_layout_extent(uint32_t n_streams, uint32_t w, uint32_t h, const h263mi_yuv_layout *lay, uint64_t *bytes, YuvLayout *shape,
                      std::vector<uint64_t> *offsets_out)
{
    if (!n_streams || !w || !h || w > 65535 || h > 65535) return H263MI_ERR_INVALID_ARGUMENT;
    const uint32_t fmt = lay ? lay->format : (uint32_t)H263MI_YUV_I420;
    if (fmt != H263MI_YUV_I420 && fmt != H263MI_YUV_NV12) return H263MI_ERR_INVALID_ARGUMENT;
    if (lay)
        for (uint8_t r : lay->reserved)
            if (r) return H263MI_ERR_INVALID_ARGUMENT;
    const bool nv12 = fmt == H263MI_YUV_NV12;
    const uint64_t cw = (w + 1) / 2, ch = (h + 1) / 2;
    const uint64_t row_y = w, row_c = nv12 ? 2 * cw : cw;
    const uint64_t pitch_y = (lay && lay->pitch_y) ? lay->pitch_y : row_y, pitch_c = (lay && lay->pitch_c) ? lay->pitch_c : row_c;
    if (!plane_fits(pitch_y, row_y, h) || !plane_fits(pitch_c, row_c, ch)) return H263MI_ERR_INVALID_ARGUMENT;
    const uint64_t *oy = lay ? lay->offsets_y : nullptr, *ocb = lay ? lay->offsets_cb : nullptr, *ocr = lay ? lay->offsets_cr : nullptr;
    if (nv12 && ocr) return H263MI_ERR_INVALID_ARGUMENT;
    const int given = (oy ? 1 : 0) + (ocb ? 1 : 0) + (ocr ? 1 : 0), all = nv12 ? 2 : 3;
    if (given != 0 && given != all) return H263MI_ERR_INVALID_ARGUMENT;
    const uint32_t chroma_planes = nv12 ? 1u : 2u;
    std::vector<uint64_t> offs((size_t)3 * n_streams);
    uint64_t total = 0;
    if (!given) {
        // planes back to back, pictures back to back: P bytes each
        const unsigned __int128 P = (unsigned __int128)h * pitch_y + (unsigned __int128)chroma_planes * ch * pitch_c;
        if (P * n_streams > UINT64_MAX) return H263MI_ERR_INVALID_ARGUMENT;
        for (uint32_t i = 0; i < n_streams; i++) {
            const uint64_t base = (uint64_t)P * i;
            offs[3 * i + 0] = base;
            offs[3 * i + 1] = base + h * pitch_y;
            offs[3 * i + 2] = nv12 ? offs[3 * i + 1] : base + h * pitch_y + ch * pitch_c;
        }
        total = (uint64_t)(P * n_streams);
    } else {
        std::vector<PlaneRect> planes;
        for (uint32_t i = 0; i < n_streams; i++) {
            offs[3 * i + 0] = oy[i];
            offs[3 * i + 1] = ocb[i];
            offs[3 * i + 2] = nv12 ? ocb[i] : ocr[i];
            planes.push_back(PlaneRect{pitch_y, row_y, h, oy[i], 1, false});
            for (uint32_t k = 1; k <= chroma_planes; k++) planes.push_back(PlaneRect{pitch_c, row_c, ch, offs[3 * i + k], 1, true});
        }
        RC_TRY(planes_extent(std::move(planes), &total));
    }
    if (bytes) *bytes = total;
    if (shape) {
        shape->format = nv12 ? YUV_OUT_NV12 : YUV_OUT_I420;
        shape->pitch_y = kernel_pitch(pitch_y, row_y, h);
        shape->pitch_c = kernel_pitch(pitch_c, row_c, ch);
        shape->bytes = total;
        bool wide = shape->pitch_y % 4 == 0 && shape->pitch_c % 4 == 0;
        for (uint64_t o : offs) wide = wide && o % 4 == 0;
        shape->wide = wide;
    }
    if (offsets_out) *offsets_out = std::move(offs);
    return H263MI_OK;
}

h263mi_rgba_layout layout_of(const h263mi_rgba_resize &r)
{
    h263mi_rgba_layout lay{};
    lay.row_pitch = r.row_pitch;
    lay.offsets = r.offsets;
    return lay;
}

h263mi_yuv_layout layout_of(const h263mi_yuv_resize &r)
{
    h263mi_yuv_layout lay{};
    lay.format = r.format;
    lay.pitch_y = r.pitch_y;
    lay.pitch_c = r.pitch_c;
    lay.offsets_y = r.offsets_y;
    lay.offsets_cb = r.offsets_cb;
    lay.offsets_cr = r.offsets_cr;
    return lay;
}

// what a resize must say before the rules of a layout apply to it
template <typename R>
static bool resize_named(const R *r)
{
    if (!r || !r->out_width || !r->out_height) return false;
    for (uint8_t v : r->reserved)
        if (v) return false;
    return true;
}

int rgba_resize_extent(uint32_t n_streams, const h263mi_rgba_resize *r, uint64_t *bytes)
{
    if (!resize_named(r)) return H263MI_ERR_INVALID_ARGUMENT;
    const h263mi_rgba_layout lay = layout_of(*r);
    return rgba_layout_extent(n_streams, r->out_width, r->out_height, &lay, nullptr, nullptr, bytes);
}

int yuv_resize_extent(uint32_t n_streams, const h263mi_yuv_resize *r, uint64_t *bytes, YuvLayout *shape, std::vector<uint64_t> *offsets)
{
    if (!resize_named(r)) return H263MI_ERR_INVALID_ARGUMENT;
    const h263mi_yuv_layout lay = layout_of(*r);
    return yuv_layout_extent(n_streams, r->out_width, r->out_height, &lay, bytes, shape, offsets);
}

// h263mi_tensor_extent (include/h263mi.h has the rules); every sum in 128 bits, so nothing wraps
int tensor_extent(uint32_t n_streams, const h263mi_tensor_out *t, uint64_t *bytes, RgbaLayout::Resize::Tensor *out, uint64_t *stride_n_out)
{
    typedef unsigned __int128 u128;
    if (!t || !n_streams || !t->out_width || !t->out_height) return H263MI_ERR_INVALID_ARGUMENT;
    if (t->dtype > H263MI_TENSOR_BF16 || t->bgr > 1 || t->reserved[0] || t->reserved[1]) return H263MI_ERR_INVALID_ARGUMENT;
    for (int c = 0; c < 3; c++)
        if (!std::isfinite(t->scale[c]) || !std::isfinite(t->bias[c])) return H263MI_ERR_INVALID_ARGUMENT;
    const uint64_t elt = t->dtype == H263MI_TENSOR_F32 ? 4 : 2, W = t->out_width, H = t->out_height;
    const uint64_t stride_h = t->stride_h ? t->stride_h : W;
    if (stride_h < W) return H263MI_ERR_INVALID_ARGUMENT;
    const u128 plane = (u128)(H - 1) * stride_h + W;          // elements from a plane's first to behind its last
    const u128 stride_c = t->stride_c ? (u128)t->stride_c : (u128)H * stride_h;
    if (stride_c < plane) return H263MI_ERR_INVALID_ARGUMENT;
    const u128 picture = 2 * stride_c + plane;
    if (picture * elt >= ((u128)1 << 32)) return H263MI_ERR_INVALID_ARGUMENT;
    const u128 stride_n = t->stride_n ? (u128)t->stride_n : 3 * stride_c;
    if (n_streams > 1 && stride_n < picture) return H263MI_ERR_INVALID_ARGUMENT;
    const u128 total = ((u128)(n_streams - 1) * stride_n + picture) * elt;
    // (the streams' byte offsets must fit too: they are below `total`)
    if (total > UINT64_MAX) return H263MI_ERR_INVALID_ARGUMENT;
    if (bytes) *bytes = (uint64_t)total;
    if (out) {
        out->on = true;
        out->dtype = t->dtype;
        out->bgr = t->bgr;
        out->elt = (uint32_t)elt;
        for (int c = 0; c < 3; c++) out->scale[c] = t->scale[c], out->bias[c] = t->bias[c];
        out->stride_c = (uint64_t)stride_c;
        out->stride_h = stride_h;
    }
    if (stride_n_out) *stride_n_out = n_streams > 1 ? (uint64_t)stride_n : 0;
    return H263MI_OK;
}

// h263mi_framing_resolve (include/h263mi.h has the rules): exact integer arithmetic, every product below 2^32
static uint32_t rnd_div(uint64_t a, uint64_t b) { return (uint32_t)((2 * a + b) / (2 * b)); }
static uint32_t clamp_to(uint32_t v, uint32_t hi) { return v < 1 ? 1 : (v > hi ? hi : v); }

int framing_resolve(uint32_t w, uint32_t h, uint32_t ow, uint32_t oh, const h263mi_framing *f, h263mi_framing_rects *out, bool *whole)
{
    if (!out || !w || !h || !ow || !oh || w > 65535 || h > 65535 || ow > 65535 || oh > 65535) return H263MI_ERR_INVALID_ARGUMENT;
    const uint32_t mode = f ? f->mode : (uint32_t)H263MI_FRAME_STRETCH;
    uint32_t sx = 0, sy = 0, sw = w, sh = h, dx = 0, dy = 0, dw = ow, dh = oh;
    if (f) {
        if (mode > H263MI_FRAME_WINDOW || f->keep_outside > 1) return H263MI_ERR_INVALID_ARGUMENT;
        for (uint8_t r : f->reserved)
            if (r) return H263MI_ERR_INVALID_ARGUMENT;
        const bool any = f->src_x || f->src_y || f->src_w || f->src_h || f->dst_x || f->dst_y || f->dst_w || f->dst_h;
        if (mode != H263MI_FRAME_WINDOW && any) return H263MI_ERR_INVALID_ARGUMENT;
    }
    const bool wide = (uint64_t)w * oh >= (uint64_t)h * ow;        // the picture's aspect is at least the output's
    if (mode == H263MI_FRAME_LETTERBOX) {
        if (wide) dh = clamp_to(rnd_div((uint64_t)h * ow, w), oh);
        else dw = clamp_to(rnd_div((uint64_t)w * oh, h), ow);
        dx = (ow - dw) / 2;
        dy = (oh - dh) / 2;
    } else if (mode == H263MI_FRAME_COVER) {
        if (wide) sw = clamp_to(rnd_div((uint64_t)h * ow, oh), w);
        else sh = clamp_to(rnd_div((uint64_t)w * oh, ow), h);
        sx = (w - sw) / 2;
        sy = (h - sh) / 2;
    } else if (mode == H263MI_FRAME_WINDOW) {
        sx = f->src_x, sy = f->src_y, sw = f->src_w, sh = f->src_h;
        dx = f->dst_x, dy = f->dst_y, dw = f->dst_w, dh = f->dst_h;
        if (!sw || !sh || !dw || !dh || sx + sw > w || sy + sh > h || dx + dw > ow || dy + dh > oh) return H263MI_ERR_INVALID_ARGUMENT;
    }
    *out = h263mi_framing_rects{(uint16_t)sx, (uint16_t)sy, (uint16_t)sw, (uint16_t)sh, (uint16_t)dx, (uint16_t)dy, (uint16_t)dw, (uint16_t)dh};
    if (whole) *whole = sw == w && sh == h && dw == ow && dh == oh;
    return H263MI_OK;
}

// the framing of `f` for w x h -> ow x oh where it is NOT the unframed shape (then true, *rc filled in); f must resolve
static bool framed_rects(uint32_t w, uint32_t h, uint32_t ow, uint32_t oh, const h263mi_framing *f, h263mi_framing_rects *rc)
{
    bool whole = true;
    return f && framing_resolve(w, h, ow, oh, f, rc, &whole) == H263MI_OK && !whole;
}

int filter_kind(const h263mi_filter *flt, uint32_t *kind)
{
    if (kind) *kind = H263MI_FILTER_AREA;
    if (!flt) return H263MI_OK;
    if (flt->kind > H263MI_FILTER_BICUBIC) return H263MI_ERR_INVALID_ARGUMENT;
    for (uint8_t r : flt->reserved)
        if (r) return H263MI_ERR_INVALID_ARGUMENT;
    if (kind) *kind = flt->kind;
    return H263MI_OK;
}

// the bytes of the tap tables of `flt` (not AREA) for w x h -> ow x oh under `f` (NULL: none), which must resolve
static uint64_t filter_table_bytes(uint32_t w, uint32_t h, uint32_t ow, uint32_t oh, const h263mi_framing *f, uint32_t kind)
{
    h263mi_framing_rects rc;
    if (framing_resolve(w, h, ow, oh, f, &rc) != H263MI_OK) return 0;
    return 4 * filter_table_words(kind, rc.src_w, rc.src_h, rc.dst_w, rc.dst_h);
}

uint64_t tensor_scratch_bytes(uint32_t w, uint32_t h, uint32_t slots, const h263mi_tensor_out &t, const h263mi_framing *f,
                              const h263mi_filter *flt)
{
    uint32_t kind = H263MI_FILTER_AREA;
    if (filter_kind(flt, &kind) == H263MI_OK && kind != H263MI_FILTER_AREA)
        return (uint64_t)slots * w * h * 4 + filter_table_bytes(w, h, t.out_width, t.out_height, f, kind);
    h263mi_framing_rects rc;
    const uint64_t spans = framed_rects(w, h, t.out_width, t.out_height, f, &rc) ? (uint64_t)rc.dst_w + rc.dst_h
                                                                                 : (uint64_t)t.out_width + t.out_height;
    return (uint64_t)slots * w * h * 4 + spans * sizeof(ResizeSpan);
}

bool resize_as_layout(uint32_t w, uint32_t h, const h263mi_rgba_resize &r, h263mi_rgba_layout *lay)
{
    for (int f = 0; f <= 2; f++) {
        const uint32_t m = (1u << f) - 1;
        if ((w & m) || (h & m) || r.out_width != (w >> f) || r.out_height != (h >> f)) continue;
        *lay = layout_of(r);
        lay->scale_log2 = (uint8_t)f;
        return true;
    }
    return false;
}

uint64_t resize_scratch_bytes(uint32_t w, uint32_t h, uint32_t slots, const h263mi_rgba_resize &r, const h263mi_framing *f,
                              const h263mi_filter *flt)
{
    uint32_t kind = H263MI_FILTER_AREA;
    if (filter_kind(flt, &kind) == H263MI_OK && kind != H263MI_FILTER_AREA)
        return (uint64_t)slots * w * h * 4 + filter_table_bytes(w, h, r.out_width, r.out_height, f, kind);
    h263mi_rgba_layout lay;
    h263mi_framing_rects rc;
    if (framed_rects(w, h, r.out_width, r.out_height, f, &rc))
        return (uint64_t)slots * w * h * 4 + ((uint64_t)rc.dst_w + rc.dst_h) * sizeof(ResizeSpan);
    if (resize_as_layout(w, h, r, &lay)) return 0;
    return (uint64_t)slots * w * h * 4 + ((uint64_t)r.out_width + r.out_height) * sizeof(ResizeSpan);
}

// =========================================================================================
// shapes
// =========================================================================================
int make_rgba_layout_shape(uint32_t n, uint32_t w, uint32_t h, const h263mi_rgba_layout *layout, RgbaLayout &out)
{
    RgbaLayout lay;
    uint32_t ow = 0, oh = 0;
    RC_TRY(rgba_layout_extent(n, w, h, layout, &ow, &oh, &lay.bytes, &lay.kernel));
    if (lay.placed()) {
        lay.offsets.resize(n);
        const uint64_t pitch = (layout->row_pitch ? layout->row_pitch : 4ull * ow);
        for (uint32_t i = 0; i < n; i++) lay.offsets[i] = layout->offsets ? layout->offsets[i] : (uint64_t)i * oh * pitch;
    }
    out = std::move(lay);
    return H263MI_OK;
}

// The scratch of a resize on `device`: `pixel_bytes` for the full-size pictures, and the span tables of the geometries
// (source length -> output length, in the order the kernel's tables lie) uploaded.
struct SpanGeometry { uint32_t in, out, at = 0; };      // (at: where the `in` source columns start -- a framing's source window)
static int make_scratch(int device, size_t pixel_bytes, std::initializer_list<SpanGeometry> geometries, std::shared_ptr<ResizeScratch> &out)
{
    std::vector<ResizeSpan> spans;
    for (const SpanGeometry &g : geometries) {
        spans.resize(spans.size() + g.out);
        resize_spans(g.in, g.out, spans.data() + spans.size() - g.out);
        for (uint32_t k = 0; k < g.out; k++) spans[spans.size() - g.out + k].first += g.at;
    }
    DeviceGuard g(device);
    if (!g.ok) return H263MI_ERR_NO_DEVICE;
    std::shared_ptr<ResizeScratch> sc(new (std::nothrow) ResizeScratch());
    if (!sc) return H263MI_ERR_OUT_OF_MEMORY;
    RC_TRY(sc->pixels.make(device, pixel_bytes));
    RC_TRY(sc->spans.make(device, spans.size() * sizeof(ResizeSpan), spans.data()));
    out = std::move(sc);
    return H263MI_OK;
}

// The framing `f` of a w x h picture in an ow x oh output, validated; where it is not the unframed shape: into `fr`, and the
// geometries of its span tables into g[2] (else fr.on stays false and g is that of the plain resize)
static int resolve_framed(uint32_t w, uint32_t h, uint32_t ow, uint32_t oh, const h263mi_framing *f, RgbaLayout::Resize::Framed &fr,
                          SpanGeometry g[2])
{
    g[0] = SpanGeometry{w, ow};
    g[1] = SpanGeometry{h, oh};
    if (!f) return H263MI_OK;
    h263mi_framing_rects rc;
    bool whole = true;
    RC_TRY(framing_resolve(w, h, ow, oh, f, &rc, &whole));
    if (whole) return H263MI_OK;
    // (kernels.h: only a stub runtime lacks the framed kernels)
    if (!launch_rgba_resize_framed || !launch_tensor_resize_framed) return H263MI_ERR_HIP;
    fr.on = true;
    fr.rc = rc;
    fr.pad = (uint32_t)f->pad[0] | (uint32_t)f->pad[1] << 8 | (uint32_t)f->pad[2] << 16;
    fr.keep = f->keep_outside != 0;
    g[0] = SpanGeometry{rc.src_w, rc.dst_w, rc.src_x};
    g[1] = SpanGeometry{rc.src_h, rc.dst_h, rc.src_y};
    return H263MI_OK;
}

// The resize of `shape` under the filter `kind` (not AREA): the framing resolved (whole onto whole without one), the scratch
// with the full-size pictures and the tap tables of the rectangles
static int make_filtered(int device, uint32_t n, uint32_t w, uint32_t h, uint32_t ow, uint32_t oh, const h263mi_framing *f, uint32_t kind,
                         RgbaLayout &shape)
{
    h263mi_framing_rects rc;
    bool whole = true;
    RC_TRY(framing_resolve(w, h, ow, oh, f, &rc, &whole));
    // (kernels.h: only a stub runtime lacks the filter kernels)
    if (!launch_rgba_filter || !launch_tensor_filter) return H263MI_ERR_HIP;
    RgbaLayout::Resize &rz = shape.resize;
    rz.framed.on = !whole;
    rz.framed.rc = rc;
    if (f) {
        rz.framed.pad = (uint32_t)f->pad[0] | (uint32_t)f->pad[1] << 8 | (uint32_t)f->pad[2] << 16;
        rz.framed.keep = f->keep_outside != 0;
    }
    const FilterTable table = filter_table(kind, rc.src_x, rc.src_y, rc.src_w, rc.src_h, rc.dst_w, rc.dst_h);
    DeviceGuard g(device);
    if (!g.ok) return H263MI_ERR_NO_DEVICE;
    std::shared_ptr<ResizeScratch> sc(new (std::nothrow) ResizeScratch());
    if (!sc) return H263MI_ERR_OUT_OF_MEMORY;
    RC_TRY(sc->pixels.make(device, (size_t)n * w * h * 4));
    RC_TRY(sc->spans.make(device, table.words.size() * sizeof(uint32_t), table.words.data()));
    rz.scratch = std::move(sc);
    rz.filter.on = true;
    rz.filter.kind = kind;
    rz.filter.ksx = table.ksx;
    rz.filter.ksy = table.ksy;
    rz.ow = ow;
    rz.oh = oh;
    return H263MI_OK;
}

int make_output_shape(int device, uint32_t n, uint32_t w, uint32_t h, const h263mi_rgba_resize *r, RgbaLayout &out, const h263mi_framing *f,
                      const h263mi_filter *flt)
{
    if (!r) return make_rgba_layout_shape(n, w, h, nullptr, out);
    RgbaLayout shape;
    RC_TRY(rgba_resize_extent(n, r, &shape.bytes));
    const uint32_t ow = r->out_width, oh = r->out_height;
    uint32_t kind = H263MI_FILTER_AREA;
    RC_TRY(filter_kind(flt, &kind));
    if (kind != H263MI_FILTER_AREA) {
        const uint64_t row = 4ull * ow, pitch = r->row_pitch ? r->row_pitch : row;
        RC_TRY(make_filtered(device, n, w, h, ow, oh, f, kind, shape));
        shape.offsets.resize(n);
        for (uint32_t i = 0; i < n; i++) shape.offsets[i] = r->offsets ? r->offsets[i] : (uint64_t)i * oh * pitch;
        shape.resize.pitch = kernel_pitch(pitch, row, oh);
        out = std::move(shape);
        return H263MI_OK;
    }
    SpanGeometry g[2];
    RC_TRY(resolve_framed(w, h, ow, oh, f, shape.resize.framed, g));
    h263mi_rgba_layout lay;
    // identical by definition: the fused layout kernels, no scratch, no extra pass
    if (!shape.resize.framed.on && resize_as_layout(w, h, *r, &lay)) return make_rgba_layout_shape(n, w, h, &lay, out);
    const uint64_t row = 4ull * ow, pitch = r->row_pitch ? r->row_pitch : row;
    RC_TRY(make_scratch(device, (size_t)n * w * h * 4, {g[0], g[1]}, shape.resize.scratch));
    shape.offsets.resize(n);
    for (uint32_t i = 0; i < n; i++) shape.offsets[i] = r->offsets ? r->offsets[i] : (uint64_t)i * oh * pitch;
    shape.resize.ow = ow;
    shape.resize.oh = oh;
    shape.resize.pitch = kernel_pitch(pitch, row, oh);
    out = std::move(shape);
    return H263MI_OK;
}

int make_tensor_shape(int device, uint32_t n, uint32_t w, uint32_t h, const h263mi_tensor_out *t, RgbaLayout &out, const h263mi_framing *f,
                      const h263mi_filter *flt)
{
    if (!t) return make_rgba_layout_shape(n, w, h, nullptr, out);
    RgbaLayout shape;
    uint64_t stride_n = 0;
    RC_TRY(tensor_extent(n, t, &shape.bytes, &shape.resize.tensor, &stride_n));
    uint32_t kind = H263MI_FILTER_AREA;
    RC_TRY(filter_kind(flt, &kind));
    if (kind != H263MI_FILTER_AREA) {
        RC_TRY(make_filtered(device, n, w, h, t->out_width, t->out_height, f, kind, shape));
        shape.offsets.resize(n);
        for (uint32_t i = 0; i < n; i++) shape.offsets[i] = (uint64_t)i * stride_n * shape.resize.tensor.elt;
        out = std::move(shape);
        return H263MI_OK;
    }
    SpanGeometry g[2];
    RC_TRY(resolve_framed(w, h, t->out_width, t->out_height, f, shape.resize.framed, g));
    RC_TRY(make_scratch(device, (size_t)n * w * h * 4, {g[0], g[1]}, shape.resize.scratch));
    shape.offsets.resize(n);
    for (uint32_t i = 0; i < n; i++) shape.offsets[i] = (uint64_t)i * stride_n * shape.resize.tensor.elt;
    shape.resize.ow = t->out_width;
    shape.resize.oh = t->out_height;
    out = std::move(shape);
    return H263MI_OK;
}

int make_yuv_shape(int device, uint32_t n, uint32_t w, uint32_t h, const h263mi_yuv_layout *lay, YuvLayout &out)
{
    YuvLayout shape;
    if (!lay) {
        out = std::move(shape);
        return H263MI_OK;
    }
    std::vector<uint64_t> offs;
    RC_TRY(yuv_layout_extent(n, w, h, lay, nullptr, &shape, &offs));
    DeviceGuard g(device);
    if (!g.ok) return H263MI_ERR_NO_DEVICE;
    std::shared_ptr<DeviceBlock> d(new (std::nothrow) DeviceBlock());
    if (!d) return H263MI_ERR_OUT_OF_MEMORY;
    RC_TRY(d->make(device, offs.size() * sizeof(uint64_t), offs.data()));
    shape.offsets = std::move(d);
    out = std::move(shape);
    return H263MI_OK;
}

int make_yuv_resize_shape(int device, uint32_t n, uint32_t w, uint32_t h, const h263mi_yuv_resize *r, YuvLayout &out, const h263mi_filter *flt)
{
    uint32_t kind = H263MI_FILTER_AREA;
    RC_TRY(filter_kind(flt, &kind));
    if (!r) {
        out = YuvLayout();
        return H263MI_OK;
    }
    YuvLayout placed, shape;                    // (shape.format 0: the rendering kernels write their default planes, into the scratch)
    RC_TRY(yuv_resize_extent(n, r, nullptr, &placed, &shape.resize.offsets));
    const uint32_t ow = r->out_width, oh = r->out_height;
    if (ow == w && oh == h) {                   // identical by definition: the YUV instantiations, no scratch, no extra pass
        const h263mi_yuv_layout lay = layout_of(*r);
        return make_yuv_shape(device, n, w, h, &lay, out);
    }
    const uint32_t cw = (w + 1) / 2, ch = (h + 1) / 2, cow = (ow + 1) / 2, coh = (oh + 1) / 2;
    const size_t pixel_bytes = (size_t)n * ((size_t)w * h + 2 * (size_t)cw * ch);
    if (kind != H263MI_FILTER_AREA) {
        // the tap tables of luma and chroma back to back, made once (plane_filter_kernel.inl: plane_filter_axes)
        if (!launch_plane_filter) return H263MI_ERR_HIP;       // (kernels.h: only a stub runtime lacks it)
        const FilterTable ty = filter_table(kind, 0, 0, w, h, ow, oh), tc = filter_table(kind, 0, 0, cw, ch, cow, coh);
        std::vector<uint32_t> words(ty.words);
        words.insert(words.end(), tc.words.begin(), tc.words.end());
        DeviceGuard g(device);
        if (!g.ok) return H263MI_ERR_NO_DEVICE;
        std::shared_ptr<ResizeScratch> sc(new (std::nothrow) ResizeScratch());
        if (!sc) return H263MI_ERR_OUT_OF_MEMORY;
        RC_TRY(sc->pixels.make(device, pixel_bytes));
        RC_TRY(sc->spans.make(device, words.size() * sizeof(uint32_t), words.data()));
        shape.resize.scratch = std::move(sc);
        shape.resize.filter.on = true;
        shape.resize.filter.kind = kind;
        shape.resize.filter.ksx_y = ty.ksx, shape.resize.filter.ksy_y = ty.ksy;
        shape.resize.filter.ksx_c = tc.ksx, shape.resize.filter.ksy_c = tc.ksy;
    } else {
        RC_TRY(make_scratch(device, pixel_bytes, {{w, ow}, {h, oh}, {cw, cow}, {ch, coh}}, shape.resize.scratch));
    }
    shape.bytes = placed.bytes;
    shape.resize.format = placed.format;
    shape.resize.ow = ow;
    shape.resize.oh = oh;
    shape.resize.pitch_y = placed.pitch_y;
    shape.resize.pitch_c = placed.pitch_c;
    shape.resize.wide = placed.wide;
    out = std::move(shape);
    return H263MI_OK;
}

}  // namespace h263mi

// =========================================================================================
// C ABI: what a placement comes to
// =========================================================================================
extern "C" {

int h263mi_rgba_layout_extent(uint32_t n_streams, uint16_t width, uint16_t height, const h263mi_rgba_layout *layout,
                              uint16_t *out_w, uint16_t *out_h, uint64_t *bytes)
{
    uint32_t ow = 0, oh = 0;
    RC_TRY(h263mi::rgba_layout_extent(n_streams, width, height, layout, &ow, &oh, bytes));
    if (out_w) *out_w = (uint16_t)ow;
    if (out_h) *out_h = (uint16_t)oh;
    return H263MI_OK;
}
int h263mi_yuv_layout_extent(uint32_t n_streams, uint16_t width, uint16_t height, const h263mi_yuv_layout *layout, uint64_t *bytes)
{
    return h263mi::yuv_layout_extent(n_streams, width, height, layout, bytes);
}
int h263mi_rgba_resize_extent(uint32_t n_streams, const h263mi_rgba_resize *r, uint64_t *bytes) { return h263mi::rgba_resize_extent(n_streams, r, bytes); }
int h263mi_yuv_resize_extent(uint32_t n_streams, const h263mi_yuv_resize *r, uint64_t *bytes) { return h263mi::yuv_resize_extent(n_streams, r, bytes); }
int h263mi_tensor_extent(uint32_t n_streams, const h263mi_tensor_out *t, uint64_t *bytes) { return h263mi::tensor_extent(n_streams, t, bytes); }
int h263mi_framing_resolve(uint16_t w, uint16_t h, uint16_t out_w, uint16_t out_h, const h263mi_framing *f, h263mi_framing_rects *out)
{
    return h263mi::framing_resolve(w, h, out_w, out_h, f, out);
}
int h263mi_filter_taps(uint8_t kind, uint32_t in_size, uint32_t out_size, uint32_t *ksize, uint32_t *first, uint32_t *count,
                       int32_t *coeffs, size_t coeff_capacity)
{
    if (!ksize || (kind != H263MI_FILTER_BILINEAR && kind != H263MI_FILTER_BICUBIC)) return H263MI_ERR_INVALID_ARGUMENT;
    if (!in_size || !out_size || in_size > 65535 || out_size > 65535) return H263MI_ERR_INVALID_ARGUMENT;
    const uint32_t ks = h263mi::filter_ksize(kind, in_size, out_size);
    if (coeffs) {
        if (!first || !count || coeff_capacity < (size_t)out_size * ks) return H263MI_ERR_INVALID_ARGUMENT;
        h263mi::filter_taps(kind, in_size, out_size, ks, first, count, coeffs);
    }
    *ksize = ks;
    return H263MI_OK;
}

}  // extern "C"
