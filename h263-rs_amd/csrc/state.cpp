// state.cpp -- the H263State mirror (h263/src/decoder/state.rs:16-490): a batch of one stream fed with host records or
// coded pictures, its DecodedPicture accessors (picture.rs:61-142) and the rendering a consumer composes behind them.
#include "batch.h"

#include <algorithm>
#include <cstring>
#include <memory>
#include <new>

using namespace h263mi;

struct h263mi_state {
    uint32_t options = 0;
    h263mi_backend_cfg cfg{};
    h263mi_batch *b = nullptr;
    h263mi_picture_desc last_desc{};
    bool has_last = false;
    bits::ParserContext parser_ctx;   // header + format of the last picture decoded from a bitstream (state.rs:143-167)
    bits::ParsedPicture parsed;       // parse results of h263mi_decode_next_picture: kept, so that its buffers are reused
    DeviceBlock rgba, planes;         // grow-only scratches: what the h263mi_render_rgba* / h263mi_render_yuv* entries render into
    // h263mi_render_yuv: the device-side shape it renders in (per format: 256-byte pitches, the wide-store path for every
    // picture size), kept for as long as the picture size stays, and the scratch that holds the planes
    struct YuvScratch {
        h263mi_batch::YuvLayout shape;
        uint32_t w = 0, h = 0;
    } yuv[2];
    ~h263mi_state()
    {
        DeviceGuard g(cfg.device_id);
        if (b) (void)hipStreamSynchronize(b->stream);
        delete b;
    }
};

// state.rs:421-483 from host records; the coefficients come either as dense blocks (`coeffs`) or as events
// (`first_event` + `events`, expanded on the device).  Staged and launched by the batch's host path (batch_submit_host).
static int submit_records(h263mi_state *s, const h263mi_picture_desc *desc, const h263mi_mb_record *mbs, size_t n_mbs,
                          const int16_t *coeffs, size_t n_coeff_blocks, const uint32_t *first_event, const uint32_t *events,
                          size_t n_events, bool validated = false);

extern "C" {

int h263mi_state_new(uint32_t decoder_options, const h263mi_backend_cfg *cfg, h263mi_state **out)
{
    if (!out) return H263MI_ERR_INVALID_ARGUMENT;
    const int dev = cfg ? cfg->device_id : 0;
    RC_TRY(check_device(dev));
    h263mi_state *s = new (std::nothrow) h263mi_state();
    if (!s) return H263MI_ERR_OUT_OF_MEMORY;
    s->options = decoder_options;
    if (cfg) s->cfg = *cfg;
    s->cfg.device_id = dev;
    s->cfg.flags &= ~(H263MI_CFG_OVERLAP_POST | H263MI_CFG_PIPELINE_POST);   // batches only: h263mi_render_rgba copies back on the main stream
    *out = s;
    return H263MI_OK;
}

void h263mi_state_free(h263mi_state *s) { delete s; }

int h263mi_state_is_sorenson(const h263mi_state *s) { return s && (s->options & H263MI_SORENSON_SPARK_BITSTREAM) ? 1 : 0; }

int h263mi_state_reset(h263mi_state *s)
{
    if (!s) return H263MI_ERR_INVALID_ARGUMENT;
    s->has_last = false;
    s->parser_ctx = bits::ParserContext();
    if (s->b) {
        DeviceGuard g(s->b->device);
        return s->b->forget_pictures();
    }
    return H263MI_OK;
}

int h263mi_state_cleanup_buffers(h263mi_state *s)
{
    // The store never holds more than the last and the reference picture (two frame sets),
    // which is exactly what cleanup_buffers (state.rs:81-98) leaves behind.
    return s ? H263MI_OK : H263MI_ERR_INVALID_ARGUMENT;
}

}  // extern "C"

static int submit_records(h263mi_state *s, const h263mi_picture_desc *desc, const h263mi_mb_record *mbs, size_t n_mbs,
                          const int16_t *coeffs, size_t n_coeff_blocks, const uint32_t *first_event, const uint32_t *events,
                          size_t n_events, bool validated)
{
    // validated: the arrays are what bits::parse_picture just wrote -- valid by construction (quantisers, types, block
    // indices, one event per position), so the checks a caller's arrays get are skipped
    const bool sparse = first_event != nullptr;
    if (!s || !desc || (!mbs && n_mbs) || (!sparse && !coeffs && n_coeff_blocks) || (sparse && !events && n_events))
        return H263MI_ERR_INVALID_ARGUMENT;
    // what the batch's host path takes of one stream
    if (n_coeff_blocks > kMaxStreamBlocks || n_events > kMaxEventWords) return H263MI_ERR_INVALID_ARGUMENT;
    if (sparse && !validated && !events_valid(first_event, n_coeff_blocks, events, n_events)) return H263MI_ERR_INVALID_ARGUMENT;
    if (!desc->width || !desc->height || !layout_fits(desc->width, desc->height)) return H263MI_ERR_PICTURE_FORMAT_INVALID;
    if (desc->picture_type > H263MI_PICTURE_RESERVED) return H263MI_ERR_INVALID_ARGUMENT;
    const FrameLayout L = make_layout(desc->width, desc->height);
    const size_t total = (size_t)L.mbw * L.mbh;
    if (n_mbs > total) return H263MI_ERR_INVALID_ARGUMENT;

    // ---- everything that can fail is checked before any state changes (state.rs:142, 464-487)
    if (!validated && !records_valid(mbs, n_mbs, n_coeff_blocks)) return H263MI_ERR_INVALID_ARGUMENT;
    bool any_inter = n_mbs < total;   // missing macroblocks are padded as Inter (state.rs:421-427)
    for (size_t i = 0; i < n_mbs && !any_inter; i++) any_inter = mb_is_inter(mbs[i].mb_type);
    const bool same_size = s->b && s->b->L.width == L.width && s->b->L.height == L.height;
    const bool has_ref = s->b && s->b->ss[0].has_ref && s->b->ss[0].cur >= 0;
    if (any_inter && !has_ref) return H263MI_ERR_UNCODED_IFRAME_BLOCKS;              // gather.rs:149
    // A size change under inter prediction indexes the new planes with the reference's strides in
    // the reference (gather.rs:150,183: out-of-bounds panic or garbage); reported as an error here.
    if (any_inter && !same_size) return H263MI_ERR_PICTURE_FORMAT_INVALID;

    DeviceGuard g(s->cfg.device_id);
    if (!g.ok) return H263MI_ERR_NO_DEVICE;
    // A picture of another size gets a frame store of its own.  The old one -- the state's last picture -- is given up only
    // once the new picture's launch has been queued: everything from here to there can fail (allocations, copies, the
    // launch), and the reference mutates its state after the last fallible call only (state.rs:464-487).
    std::unique_ptr<h263mi_batch> fresh;
    if (!same_size) {
        h263mi_batch *nb = nullptr;
        RC_TRY(batch_create(1, L.width, L.height, &s->cfg, &nb));
        fresh.reset(nb);
    }
    // (the counts fit: n_mbs <= total, and the caps above)
    const uint32_t n_mbs32 = (uint32_t)n_mbs, blocks32 = (uint32_t)n_coeff_blocks, events32 = (uint32_t)n_events;
    RC_TRY(batch_submit_host(same_size ? s->b : fresh.get(), desc->picture_type, &mbs, &n_mbs32, &coeffs, &blocks32,
                             sparse ? &first_event : nullptr, &events, &events32, /*validated=*/true));
    // ---- the launch is queued: from here on nothing fails any more, the state changes (state.rs:464-483)
    if (fresh) {
        delete s->b;
        s->b = fresh.release();
    }
    s->last_desc = *desc;
    s->has_last = true;
    return H263MI_OK;
}

extern "C" {

int h263mi_submit_picture(h263mi_state *s, const h263mi_picture_desc *desc, const h263mi_mb_record *mbs, size_t n_mbs,
                          const int16_t *coeffs, size_t n_coeff_blocks)
{
    return submit_records(s, desc, mbs, n_mbs, coeffs, n_coeff_blocks, nullptr, nullptr, 0);
}

int h263mi_submit_picture_events(h263mi_state *s, const h263mi_picture_desc *desc, const h263mi_mb_record *mbs,
                                 size_t n_mbs, const uint32_t *block_first_event, size_t n_coeff_blocks,
                                 const uint32_t *events, size_t n_events)
{
    if (!block_first_event) return H263MI_ERR_INVALID_ARGUMENT;
    if (n_coeff_blocks > 0xffffffffu / 8u) return H263MI_ERR_INVALID_ARGUMENT;
    return submit_records(s, desc, mbs, n_mbs, nullptr, n_coeff_blocks, block_first_event, events, n_events);
}

int h263mi_decode_next_picture(h263mi_state *s, const uint8_t *data, size_t len, size_t *consumed)
{
    if (!s || (!data && len)) return H263MI_ERR_INVALID_ARGUMENT;
    if (consumed) *consumed = 0;
    // serial half on the host (state.rs:143-427) ...
    bits::ParsedPicture &pic = s->parsed;                // (kept between calls: no allocation per picture)
    prepare_for_parse(pic, /*sparse=*/false);
    if (s->b) {
        // A stream rarely changes its size: the records are parsed straight into the batch's staging slot the next submit
        // copies from (sized for the last picture; a picture with more macroblocks falls back to the parser's own array).
        // The slot was last read by the copy of two pictures ago.
        DeviceGuard g(s->cfg.device_id);
        h263mi_batch::HostStaging &g2 = s->b->host_stg[s->b->host_slot & 1];
        if (g.ok && s->b->ensure_record_staging(g2) == H263MI_OK && hipEventSynchronize(g2.done) == hipSuccess) {
            pic.mbs_ext = g2.mbs.h;
            pic.mbs_ext_cap = (size_t)s->b->L.mbw * s->b->L.mbh;
        }
    }
    RC_TRY(bits::parse_picture(data, len, s->options, &s->parser_ctx, pic));
    // ... everything from the cut line on (state.rs:421-483) on the GPU.  Nothing has touched the state so
    // far, so every error above leaves it unchanged, like the reader transaction of state.rs:142.
    if (pic.n_coded_blocks > 0xffffffffu / 8u) return H263MI_ERR_INVALID_ARGUMENT;
    RC_TRY(submit_records(s, &pic.desc, pic.records(), pic.n_records(), nullptr, pic.n_coded_blocks, pic.block_first_event.data(),
                          pic.events.data(), pic.events.size(), /*validated=*/true));
    s->parser_ctx = pic.next;
    if (consumed) *consumed = pic.bits_consumed / 8;     // reader.commit() drains whole bytes (reader.rs:391-394)
    return H263MI_OK;
}

int h263mi_parse_picture_header(const h263mi_state *s, const uint8_t *data, size_t len, h263mi_picture_desc *out)
{
    if (!s || !out || (!data && len)) return H263MI_ERR_INVALID_ARGUMENT;
    bits::BitReader r(data, len);
    bits::PictureHeader h;
    bool is_picture = false;
    RC_TRY(bits::decode_picture_header(r, s->options, &s->parser_ctx, h, is_picture));
    if (!is_picture) return H263MI_ERR_MIDDLE_OF_BITSTREAM;
    memset(out, 0, sizeof *out);
    out->width = h.width;
    out->height = h.height;
    out->picture_type = h.picture_type;
    out->pquant = h.quantizer;
    out->use_deblocker = h.use_deblocker ? 1 : 0;
    out->temporal_reference = h.temporal_reference;
    return H263MI_OK;
}

static int fill_view(const h263mi_state *s, h263mi_frame_view *out)
{
    const h263mi_batch *b = s->b;
    const uint8_t *f = b->frames[b->ss[0].cur];
    memset(out, 0, sizeof *out);
    out->width = (uint16_t)b->L.width;
    out->height = (uint16_t)b->L.height;
    out->chroma_width = (uint16_t)b->L.cwidth;
    out->chroma_height = (uint16_t)b->L.cheight;
    out->temporal_reference = s->last_desc.temporal_reference;
    out->picture_type = s->last_desc.picture_type;
    out->pquant = s->last_desc.pquant;
    out->use_deblocker = s->last_desc.use_deblocker;
    out->dev_y = f;
    out->dev_cb = f + b->L.off_cb;
    out->dev_cr = f + b->L.off_cr;
    out->dev_pitch_y = b->L.pitch_y;
    out->dev_pitch_c = b->L.pitch_c;
    return H263MI_OK;
}

int h263mi_get_last_picture(const h263mi_state *s, h263mi_frame_view *out)
{
    if (!s || !out) return H263MI_ERR_INVALID_ARGUMENT;
    if (!s->has_last || !s->b || s->b->ss[0].cur < 0) return H263MI_ERR_NO_PICTURE;
    return fill_view(s, out);
}

int h263mi_get_reference_picture(const h263mi_state *s, h263mi_frame_view *out)
{
    if (!s || !out) return H263MI_ERR_INVALID_ARGUMENT;
    // state.rs:72-78: None without a reference, otherwise the entry of *last_picture*
    if (!s->has_last || !s->b || s->b->ss[0].cur < 0 || !s->b->ss[0].has_ref) return H263MI_ERR_NO_PICTURE;
    return fill_view(s, out);
}

int h263mi_copy_yuv(const h263mi_state *s, uint8_t *y, uint8_t *cb, uint8_t *cr)
{
    if (!s) return H263MI_ERR_INVALID_ARGUMENT;
    if (!s->has_last || !s->b) return H263MI_ERR_NO_PICTURE;
    DeviceGuard g(s->cfg.device_id);
    return s->b->copy_yuv(0, y, cb, cr);
}

int h263mi_digest_yuv(const h263mi_state *s, uint32_t seed, uint32_t *digest)
{
    if (!s || !digest || !digest_seed_valid(seed)) return H263MI_ERR_INVALID_ARGUMENT;
    if (!s->has_last || !s->b) return H263MI_ERR_NO_PICTURE;
    DeviceGuard g(s->cfg.device_id);
    return digest_rc(s->b->digest_yuv(seed, digest, nullptr));
}

int h263mi_change_last(const h263mi_state *s, const h263mi_plane_set *prev, const h263mi_change *c, uint32_t *d_cells, uint64_t cells_bytes,
                       h263mi_change_summary *d_summary, uint32_t *d_selected, uint32_t *d_count)
{
    if (!s) return H263MI_ERR_INVALID_ARGUMENT;
    if (!s->has_last || !s->b) return H263MI_ERR_NO_PICTURE;
    DeviceGuard g(s->cfg.device_id);
    return s->b->change_last(prev, c, d_cells, cells_bytes, d_summary, d_selected, d_count, nullptr);
}

int h263mi_background_last(const h263mi_state *s, const h263mi_background *bg, void *d_state, uint64_t state_bytes, const uint32_t *d_cut,
                           const uint32_t *d_cut_count, const h263mi_plane_set *mask, uint32_t *d_cells, uint64_t cells_bytes,
                           h263mi_change_summary *d_summary, uint32_t *d_selected, uint32_t *d_count)
{
    if (!s) return H263MI_ERR_INVALID_ARGUMENT;
    if (!s->has_last || !s->b) return H263MI_ERR_NO_PICTURE;
    DeviceGuard g(s->cfg.device_id);
    return s->b->background_last(bg, d_state, state_bytes, d_cut, d_cut_count, mask, d_cells, cells_bytes, d_summary, d_selected, d_count,
                                 nullptr);
}

int h263mi_hist_last(const h263mi_state *s, uint32_t plane, const h263mi_hist *h, uint32_t *d_hist, uint64_t hist_bytes, uint32_t *d_prev_hist,
                     uint64_t prev_bytes, h263mi_hist_stats *d_stats, uint32_t *d_selected, uint32_t *d_count)
{
    if (!s) return H263MI_ERR_INVALID_ARGUMENT;
    if (!s->has_last || !s->b) return H263MI_ERR_NO_PICTURE;
    DeviceGuard g(s->cfg.device_id);
    return s->b->hist_last(plane, h, d_hist, hist_bytes, d_prev_hist, prev_bytes, d_stats, d_selected, d_count, nullptr);
}

// `strength` of the rendering calls: 0..12, or H263MI_STRENGTH_FROM_HEADER = what the last picture's own header asks for
// (QUANT_TO_STRENGTH[quantizer] when USE_DEBLOCKER is set: deblock.rs:5-8, picture.rs:61-64)
static int state_strength(const h263mi_state *s, uint8_t strength, h263mi_batch::Strengths &st)
{
    if (strength == H263MI_STRENGTH_FROM_HEADER) {
        st.uniform = strength_from_header(s->last_desc);
        return H263MI_OK;
    }
    if (strength > 12) return H263MI_ERR_INVALID_ARGUMENT;
    st.uniform = strength;
    return H263MI_OK;
}

// The last picture as W' x H' RGBA in `shape`: rendered with tight rows into the state's scratch (which holds them), then copied out
// at the caller's pitch -- row by row when that is wider -- and waited for.
// A framing with keep_outside writes its destination rectangle alone: that rectangle alone is copied out.
static int render_rgba_shaped(h263mi_state *s, const h263mi_batch::Strengths &st, const h263mi_batch::RgbaLayout &shape, uint32_t ow,
                              uint32_t oh, uint64_t row_pitch, uint8_t *rgba)
{
    const hipStream_t on = s->b->stream;
    uint8_t *d = s->rgba.as<uint8_t>();
    RC_TRY(s->b->render(st, d, nullptr, false, nullptr, &shape));
    const size_t row = (size_t)ow * 4, pitch = row_pitch ? (size_t)row_pitch : row;
    const h263mi_batch::RgbaLayout::Resize::Framed &fr = shape.resize.framed;
    if (fr.on && fr.keep) {
        const size_t at = (size_t)fr.rc.dst_x * 4;
        HIP_TRY(hipMemcpy2DAsync(rgba + fr.rc.dst_y * pitch + at, pitch, d + fr.rc.dst_y * row + at, row, (size_t)fr.rc.dst_w * 4, fr.rc.dst_h,
                                 hipMemcpyDeviceToHost, on));
    } else if (pitch == row) HIP_TRY(hipMemcpyAsync(rgba, d, row * oh, hipMemcpyDeviceToHost, on));
    else HIP_TRY(hipMemcpy2DAsync(rgba, pitch, d, row, row, oh, hipMemcpyDeviceToHost, on));
    HIP_TRY(hipStreamSynchronize(on));
    return H263MI_OK;
}

// The last picture's planes in `shape`: rendered into the state's plane scratch (made to hold them) -- a w x h luma plane at pitch
// dpy, behind it the chroma planes (I420: Cb, Cr; NV12: one of CbCr pairs) of ch rows of row_c bytes at pitch dpc -- then each plane
// copied out row by row into the caller's rectangle (`host` has its pitches, `off` its offsets: nothing else of `out` is touched)
// and waited for.
static int render_planes_shaped(h263mi_state *s, const h263mi_batch::Strengths &st, const h263mi_batch::YuvLayout &shape, uint8_t *out,
                                const h263mi_batch::YuvLayout &host, const std::vector<uint64_t> &off, uint32_t w, uint32_t h, uint32_t row_c,
                                uint32_t ch, size_t dpy, size_t dpc)
{
    RC_TRY(s->planes.reserve(s->cfg.device_id, shape.bytes));
    RC_TRY(s->b->render(st, nullptr, s->planes.as<uint8_t>(), false, nullptr, nullptr, &shape));
    const hipStream_t on = s->b->stream;
    const uint8_t *d_y = s->planes.as<uint8_t>(), *d_c0 = d_y + (size_t)h * dpy;
    HIP_TRY(hipMemcpy2DAsync(out + off[0], h > 1 ? host.pitch_y : w, d_y, dpy, w, h, hipMemcpyDeviceToHost, on));
    HIP_TRY(hipMemcpy2DAsync(out + off[1], ch > 1 ? host.pitch_c : row_c, d_c0, dpc, row_c, ch, hipMemcpyDeviceToHost, on));
    if (host.format != YUV_OUT_NV12)
        HIP_TRY(hipMemcpy2DAsync(out + off[2], ch > 1 ? host.pitch_c : row_c, d_c0 + (size_t)ch * dpc, dpc, row_c, ch, hipMemcpyDeviceToHost, on));
    HIP_TRY(hipStreamSynchronize(on));
    return H263MI_OK;
}

int h263mi_render_rgba(const h263mi_state *cs, uint8_t strength, uint8_t *rgba)
{
    h263mi_state *s = const_cast<h263mi_state *>(cs);
    if (!s || !rgba) return H263MI_ERR_INVALID_ARGUMENT;
    if (!s->has_last || !s->b) return H263MI_ERR_NO_PICTURE;
    DeviceGuard g(s->cfg.device_id);
    h263mi_batch *b = s->b;
    RC_TRY(s->rgba.reserve(s->cfg.device_id, (size_t)b->L.width * 4 * b->L.height));
    h263mi_batch::Strengths st;
    RC_TRY(state_strength(s, strength, st));
    return render_rgba_shaped(s, st, b->layout, b->L.width, b->L.height, 0, rgba);
}

int h263mi_render_rgba_layout(const h263mi_state *cs, uint8_t strength, const h263mi_rgba_layout *layout, uint8_t *rgba)
{
    h263mi_state *s = const_cast<h263mi_state *>(cs);
    if (!s || !rgba || (layout && layout->offsets)) return H263MI_ERR_INVALID_ARGUMENT;
    if (!s->has_last || !s->b) return H263MI_ERR_NO_PICTURE;
    h263mi_batch *b = s->b;
    uint32_t ow = 0, oh = 0;
    RC_TRY(rgba_layout_extent(1, b->L.width, b->L.height, layout, &ow, &oh, nullptr));
    h263mi_batch::Strengths st;
    RC_TRY(state_strength(s, strength, st));
    DeviceGuard g(s->cfg.device_id);
    RC_TRY(s->rgba.reserve(s->cfg.device_id, (size_t)ow * 4 * oh));
    h263mi_rgba_layout tight{};
    tight.scale_log2 = layout ? layout->scale_log2 : 0;
    h263mi_batch::RgbaLayout shape;
    RC_TRY(make_rgba_layout_shape(1, b->L.width, b->L.height, &tight, shape));
    return render_rgba_shaped(s, st, shape, ow, oh, layout ? layout->row_pitch : 0, rgba);
}

int h263mi_render_rgba_resize(const h263mi_state *cs, uint8_t strength, const h263mi_rgba_resize *r, uint8_t *rgba)
{
    return h263mi_render_rgba_resize_framed(cs, strength, r, nullptr, rgba);
}

int h263mi_render_rgba_resize_framed(const h263mi_state *cs, uint8_t strength, const h263mi_rgba_resize *r, const h263mi_framing *f,
                                     uint8_t *rgba)
{
    return h263mi_render_rgba_resize_filtered(cs, strength, r, f, nullptr, rgba);
}

int h263mi_render_rgba_resize_filtered(const h263mi_state *cs, uint8_t strength, const h263mi_rgba_resize *r, const h263mi_framing *f,
                                       const h263mi_filter *flt, uint8_t *rgba)
{
    h263mi_state *s = const_cast<h263mi_state *>(cs);
    if (!s || !rgba || !r || r->offsets) return H263MI_ERR_INVALID_ARGUMENT;
    RC_TRY(filter_kind(flt));
    if (!s->has_last || !s->b) return H263MI_ERR_NO_PICTURE;
    h263mi_batch *b = s->b;
    RC_TRY(rgba_resize_extent(1, r, nullptr));
    h263mi_framing_rects rects;
    RC_TRY(framing_resolve(b->L.width, b->L.height, r->out_width, r->out_height, f, &rects));
    h263mi_batch::Strengths st;
    RC_TRY(state_strength(s, strength, st));
    DeviceGuard g(s->cfg.device_id);
    RC_TRY(s->rgba.reserve(s->cfg.device_id, (size_t)r->out_width * 4 * r->out_height));
    h263mi_rgba_resize tight = *r;
    tight.row_pitch = 0;
    h263mi_batch::RgbaLayout shape;            // (its scratch, if any, goes at the end, once the copy out has waited for it)
    RC_TRY(make_output_shape(s->cfg.device_id, 1, b->L.width, b->L.height, &tight, shape, f, flt));
    return render_rgba_shaped(s, st, shape, r->out_width, r->out_height, r->row_pitch, rgba);
}

int h263mi_render_tensor(const h263mi_state *cs, uint8_t strength, const h263mi_tensor_out *t, void *out)
{
    return h263mi_render_tensor_framed(cs, strength, t, nullptr, out);
}

int h263mi_render_tensor_framed(const h263mi_state *cs, uint8_t strength, const h263mi_tensor_out *t, const h263mi_framing *f, void *out)
{
    return h263mi_render_tensor_filtered(cs, strength, t, f, nullptr, out);
}

int h263mi_render_tensor_filtered(const h263mi_state *cs, uint8_t strength, const h263mi_tensor_out *t, const h263mi_framing *f,
                                  const h263mi_filter *flt, void *out)
{
    h263mi_state *s = const_cast<h263mi_state *>(cs);
    if (!s || !out || !t) return H263MI_ERR_INVALID_ARGUMENT;
    RC_TRY(filter_kind(flt));
    if (!s->has_last || !s->b) return H263MI_ERR_NO_PICTURE;
    h263mi_batch *b = s->b;
    // the caller's shape: where its planes lie in `out`
    h263mi_batch::RgbaLayout::Resize::Tensor host;
    RC_TRY(tensor_extent(1, t, nullptr, &host));
    h263mi_framing_rects rects;
    RC_TRY(framing_resolve(b->L.width, b->L.height, t->out_width, t->out_height, f, &rects));
    h263mi_batch::Strengths st;
    RC_TRY(state_strength(s, strength, st));
    DeviceGuard g(s->cfg.device_id);
    // written on the device as one contiguous 3 x H' x W' tensor into the state's scratch, then each plane copied out row by
    // row into the caller's rectangle
    h263mi_tensor_out tight = *t;
    tight.stride_n = tight.stride_c = tight.stride_h = 0;
    const size_t row = (size_t)t->out_width * host.elt, plane = row * t->out_height;
    RC_TRY(s->rgba.reserve(s->cfg.device_id, 3 * plane));
    h263mi_batch::RgbaLayout shape;            // (its scratch goes at the end, once the copies out have waited for it)
    RC_TRY(make_tensor_shape(s->cfg.device_id, 1, b->L.width, b->L.height, &tight, shape, f, flt));
    const uint8_t *d = s->rgba.as<uint8_t>();
    RC_TRY(b->render(st, s->rgba.as<uint8_t>(), nullptr, false, nullptr, &shape));
    const hipStream_t on = b->stream;
    // (a framing with keep_outside writes its destination rectangle alone: that rectangle alone is copied out)
    const bool rect_only = shape.resize.framed.on && shape.resize.framed.keep;
    const size_t x0 = rect_only ? rects.dst_x : 0, y0 = rect_only ? rects.dst_y : 0;
    const size_t cols = rect_only ? rects.dst_w : t->out_width, rows_out = rect_only ? rects.dst_h : t->out_height;
    for (size_t p = 0; p < 3; p++)
        HIP_TRY(hipMemcpy2DAsync(static_cast<uint8_t *>(out) + (p * host.stride_c + y0 * host.stride_h + x0) * host.elt,
                                 host.stride_h * host.elt, d + p * plane + y0 * row + x0 * host.elt, row, cols * host.elt, rows_out,
                                 hipMemcpyDeviceToHost, on));
    HIP_TRY(hipStreamSynchronize(on));
    return H263MI_OK;
}

int h263mi_render_yuv(const h263mi_state *cs, uint8_t strength, const h263mi_yuv_layout *layout, uint8_t *out)
{
    h263mi_state *s = const_cast<h263mi_state *>(cs);
    if (!s || !out) return H263MI_ERR_INVALID_ARGUMENT;
    if (!s->has_last || !s->b) return H263MI_ERR_NO_PICTURE;
    h263mi_batch *b = s->b;
    const uint32_t w = b->L.width, h = b->L.height, cw = b->L.cwidth, ch = b->L.cheight;
    // the caller's shape: where its planes lie in `out`
    h263mi_batch::YuvLayout host;
    std::vector<uint64_t> off;
    RC_TRY(yuv_layout_extent(1, w, h, layout, nullptr, &host, &off));
    h263mi_batch::Strengths st;
    RC_TRY(state_strength(s, strength, st));
    DeviceGuard g(s->cfg.device_id);
    // rendered on the device at pitches of 256 bytes, planes back to back (every layout of that kind takes the wide stores),
    // then each plane copied out row by row into the caller's rectangle
    const bool nv12 = host.format == YUV_OUT_NV12;
    const uint32_t row_c = nv12 ? 2 * cw : cw;
    const size_t dpy = ((size_t)w + 255) / 256 * 256, dpc = ((size_t)row_c + 255) / 256 * 256;
    h263mi_state::YuvScratch &sc = s->yuv[nv12 ? 1 : 0];
    if (!sc.shape.on() || sc.w != w || sc.h != h) {
        h263mi_yuv_layout dev{};
        dev.format = nv12 ? H263MI_YUV_NV12 : H263MI_YUV_I420;
        dev.pitch_y = dpy;
        dev.pitch_c = dpc;
        sc.shape = h263mi_batch::YuvLayout();
        RC_TRY(make_yuv_shape(s->cfg.device_id, 1, w, h, &dev, sc.shape));
        sc.w = w;
        sc.h = h;
    }
    return render_planes_shaped(s, st, sc.shape, out, host, off, w, h, row_c, ch, dpy, dpc);
}

int h263mi_render_yuv_resize(const h263mi_state *cs, uint8_t strength, const h263mi_yuv_resize *r, uint8_t *out)
{
    return h263mi_render_yuv_resize_filtered(cs, strength, r, nullptr, out);
}

int h263mi_render_yuv_resize_filtered(const h263mi_state *cs, uint8_t strength, const h263mi_yuv_resize *r, const h263mi_filter *flt,
                                      uint8_t *out)
{
    h263mi_state *s = const_cast<h263mi_state *>(cs);
    if (!s || !out || !r) return H263MI_ERR_INVALID_ARGUMENT;
    RC_TRY(filter_kind(flt));
    if (!s->has_last || !s->b) return H263MI_ERR_NO_PICTURE;
    h263mi_batch *b = s->b;
    // the caller's shape: where its planes lie in `out`
    h263mi_batch::YuvLayout host;
    std::vector<uint64_t> off;
    RC_TRY(yuv_resize_extent(1, r, nullptr, &host, &off));
    if (r->out_width == b->L.width && r->out_height == b->L.height) {      // the full-size layout, by definition
        const h263mi_yuv_layout lay = layout_of(*r);
        return h263mi_render_yuv(cs, strength, &lay, out);
    }
    h263mi_batch::Strengths st;
    RC_TRY(state_strength(s, strength, st));
    DeviceGuard g(s->cfg.device_id);
    // resized on the device at pitches that are multiples of 4, planes back to back (the word stores), then each plane copied
    // out row by row into the caller's rectangle
    const bool nv12 = host.format == YUV_OUT_NV12;
    const uint32_t ow = r->out_width, oh = r->out_height, cow = (ow + 1) / 2, coh = (oh + 1) / 2, row_c = nv12 ? 2 * cow : cow;
    const size_t dpy = ((size_t)ow + 3) / 4 * 4, dpc = ((size_t)row_c + 3) / 4 * 4;
    h263mi_yuv_resize dev = *r;
    dev.pitch_y = dpy;
    dev.pitch_c = dpc;
    dev.offsets_y = dev.offsets_cb = dev.offsets_cr = nullptr;
    h263mi_batch::YuvLayout shape;              // (its scratch goes at the end, once the copies out have waited for it)
    RC_TRY(make_yuv_resize_shape(s->cfg.device_id, 1, b->L.width, b->L.height, &dev, shape, flt));
    return render_planes_shaped(s, st, shape, out, host, off, ow, oh, row_c, coh, dpy, dpc);
}

int h263mi_render_rgba_pinned(const h263mi_state *cs, uint8_t strength, uint8_t *rgba_pinned)
{
    h263mi_state *s = const_cast<h263mi_state *>(cs);
    if (!s || !rgba_pinned) return H263MI_ERR_INVALID_ARGUMENT;
    if (!s->has_last || !s->b) return H263MI_ERR_NO_PICTURE;
    DeviceGuard g(s->cfg.device_id);
    h263mi_batch *b = s->b;
    // the device's view of the caller's page-locked buffer: the kernel stores RGBA straight into it
    void *dev = nullptr;
    if (hipHostGetDevicePointer(&dev, rgba_pinned, 0) != hipSuccess || !dev) {
        (void)hipGetLastError();
        return H263MI_ERR_INVALID_ARGUMENT;          // not from h263mi_host_alloc / h263mi_host_register
    }
    h263mi_batch::Strengths st;
    RC_TRY(state_strength(s, strength, st));
    RC_TRY(b->render(st, static_cast<uint8_t *>(dev), nullptr));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return H263MI_OK;
}

}  // extern "C"
