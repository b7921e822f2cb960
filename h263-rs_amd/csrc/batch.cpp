// batch.cpp -- h263mi_batch: the device-resident frame store of N streams, the reference bookkeeping of
// state.rs:464-483 per stream, submit / render / sync, launch timing, and the entry points that take DEVICE records
// (h263mi_batch_submit / _decode / _decode_events / _render_rgba / _sync ...).  Compiled with hipcc; every compute path
// launches the gfx950 kernels of the *_kernels.hip units -- there is no CPU fallback.
#include "batch.h"

#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <string>

using namespace h263mi;

// =========================================================================================
// frame store and per-stream state
// =========================================================================================
int h263mi_batch::alloc(uint32_t n_streams, uint32_t w, uint32_t h)
{
    n = n_streams;
    L = make_layout(w, h);
    // both frame sets in one allocation
    {
        const size_t set_bytes = (size_t)n * L.frame_bytes;
        // H263MI_EXP_FRAME_SKEW (experiment, a multiple of 16): the whole frame store starts that many bytes past a
        // 64-byte line, so that no row of any plane is line-aligned (profiles/README.md r03_zz: aligned RGBA runs
        // are 10 % slower than runs that start 16 bytes into a line -- the same for the planes?)
        const char *skew_env = getenv("H263MI_EXP_FRAME_SKEW");
        frame_skew = skew_env ? ((size_t)atoi(skew_env) & 0xff0u) : 0;
        HIP_TRY(hipMalloc((void **)&frames[0], 2 * set_bytes + 4096));
        frames[0] += frame_skew;
        frames[1] = frames[0] + set_bytes;
        if (getenv("H263MI_TRACE_ALLOC"))
            fprintf(stderr, "h263mi frame store: %p .. +%zu\n", (void *)frames[0], 2 * set_bytes);
        HIP_TRY(hipMemsetAsync(frames[0], 0, 2 * set_bytes, stream));
    }
    RC_TRY(status.reserve(n, 0, placement));
    RC_TRY(word_ring.make(n, placement));
    HIP_TRY(hipMemsetAsync(status.d, 0, (size_t)n * sizeof(uint32_t), stream));
    ss.assign(n, StreamState());
    pending.set.assign(n, -1);
    layout = RgbaLayout();
    layout.bytes = (uint64_t)n * w * h * 4;
    return H263MI_OK;
}

bool h263mi_batch::layout_ptrs(const RgbaLayout &lay, uint8_t *d_rgba, std::vector<uint8_t *> &ptrs) const
{
    if (!lay.placed() || !d_rgba) return false;
    ptrs.resize(n);
    for (uint32_t i = 0; i < n; i++) ptrs[i] = d_rgba + lay.offsets[i];
    return true;
}

int h263mi_batch::plane_resize_dst(const YuvLayout::Resize &rz, const std::vector<int8_t> &sets, uint8_t *d_planes, hipStream_t on,
                                   const PlaneDst **d_out, bool *wide)
{
    std::vector<PlaneDst> p(n, PlaneDst{{nullptr, nullptr, nullptr}});
    const bool nv12 = rz.format == YUV_OUT_NV12;
    for (uint32_t i = 0; i < n; i++)
        if (sets[i] >= 0) {
            p[i].p[0] = d_planes + rz.offsets[3 * i + 0];
            p[i].p[1] = d_planes + rz.offsets[3 * i + 1];
            p[i].p[2] = nv12 ? nullptr : d_planes + rz.offsets[3 * i + 2];
        }
    *wide = rz.wide && ((uintptr_t)d_planes & 3u) == 0;
    return upload(plane_ring, p.data(), d_out, on);
}

int h263mi_batch::launch_plane_resize(const YuvLayout::Resize &rz, const std::vector<int8_t> &sets, const PlaneDst *d_dst, bool wide,
                                      hipStream_t on)
{
    bool any = false;
    for (int8_t v : sets) any = any || v >= 0;
    if (!any) return H263MI_OK;
    if (rz.filter.on) {                        // Pillow's bilinear / bicubic in the place of the area average (k_plane_filter)
        PlaneFilterArgs a{};
        a.src = rz.scratch->pixels.as<uint8_t>();
        a.dst = d_dst;
        a.w = L.width, a.h = L.height, a.cw = L.cwidth, a.ch = L.cheight;
        a.ow = rz.ow, a.oh = rz.oh, a.cow = (rz.ow + 1) / 2, a.coh = (rz.oh + 1) / 2;
        plane_filter_axes(rz.scratch->spans.p, a, rz.filter.ksx_y, rz.filter.ksy_y, rz.filter.ksx_c, rz.filter.ksy_c);
        a.pitch_y = rz.pitch_y;
        a.pitch_c = rz.pitch_c;
        a.nv12 = rz.format == YUV_OUT_NV12 ? 1u : 0u;
        a.wide = wide ? 1u : 0u;
        a.d_y = L.width * L.height;
        a.d_c = L.cwidth * L.cheight;
        a.n_pictures = n;
        if (!launch_plane_filter) return H263MI_ERR_HIP;            // (kernels.h: only a stub runtime lacks it)
        RC_TRY(time_begin(5, on));
        HIP_TRY(launch_plane_filter(a, on));
        return H263MI_OK;
    }
    PlaneResizeArgs a{};
    a.src = rz.scratch->pixels.as<uint8_t>();
    a.dst = d_dst;
    a.w = L.width, a.h = L.height, a.cw = L.cwidth, a.ch = L.cheight;
    a.ow = rz.ow, a.oh = rz.oh, a.cow = (rz.ow + 1) / 2, a.coh = (rz.oh + 1) / 2;
    a.cols_y = rz.scratch->spans.as<ResizeSpan>();
    a.rows_y = a.cols_y + a.ow;
    a.cols_c = a.rows_y + a.oh;
    a.rows_c = a.cols_c + a.cow;
    a.pitch_y = rz.pitch_y;
    a.pitch_c = rz.pitch_c;
    a.nv12 = rz.format == YUV_OUT_NV12 ? 1u : 0u;
    a.wide = wide ? 1u : 0u;
    a.d_y = L.width * L.height;
    a.d_c = L.cwidth * L.cheight;
    a.inv_d_y = 1.0f / (float)a.d_y;
    a.inv_d_c = 1.0f / (float)a.d_c;
    a.n_pictures = n;
    if (!::h263mi::launch_plane_resize) return H263MI_ERR_HIP;      // (kernels.h: only a stub runtime lacks it)
    RC_TRY(time_begin(4, on));
    HIP_TRY(::h263mi::launch_plane_resize(a, on));
    return H263MI_OK;
}

int h263mi_batch::resize_dst(const RgbaLayout &lay, const std::vector<int8_t> &sets, uint8_t *d_rgba, uint8_t *const *host_ptrs,
                             hipStream_t on, uint8_t *const **d_out)
{
    std::vector<uint8_t *> p(n, nullptr);
    for (uint32_t i = 0; i < n; i++)
        if (sets[i] >= 0) p[i] = host_ptrs ? host_ptrs[i] : d_rgba + lay.offsets[i];
    return upload(ptr_ring, p.data(), d_out, on);
}

int h263mi_batch::launch_resize(const RgbaLayout::Resize &rz, const std::vector<int8_t> &sets, uint8_t *const *d_dst, hipStream_t on)
{
    bool any = false;
    for (int8_t v : sets) any = any || v >= 0;
    if (!any) return H263MI_OK;
    if (rz.filter.on) {                        // Pillow's bilinear / bicubic in the place of the area average (k_rgba_filter, k_tensor_filter)
        const h263mi_framing_rects &rc = rz.framed.rc;
        TensorFilterArgs fa{};
        FilterArgs &a = fa.fl;
        a.src = rz.scratch->pixels.as<uint8_t>();
        a.dst = d_dst;
        filter_axes(rz.scratch->spans.p, rc.dst_w, rc.dst_h, rz.filter.ksx, rz.filter.ksy, a.x, a.y);
        a.w = L.width, a.h = L.height, a.dw = rc.dst_w, a.dh = rc.dst_h;
        a.pitch = rz.pitch;
        a.n_pictures = n;
        a.f.cw = rz.ow, a.f.ch = rz.oh, a.f.dx = rc.dst_x, a.f.dy = rc.dst_y;
        a.f.pad = rz.framed.pad;
        a.f.keep = rz.framed.keep ? 1u : 0u;
        if (!launch_rgba_filter || !launch_tensor_filter) return H263MI_ERR_HIP;       // (kernels.h: only a stub runtime lacks them)
        RC_TRY(time_begin(3, on));
        if (rz.tensor.on) {
            for (int c = 0; c < 3; c++) fa.t.scale[c] = rz.tensor.scale[c], fa.t.bias[c] = rz.tensor.bias[c];
            fa.t.dtype = rz.tensor.dtype;
            fa.t.bgr = rz.tensor.bgr;
            fa.t.stride_c = rz.tensor.stride_c;
            fa.t.stride_h = rz.tensor.stride_h;
            HIP_TRY(launch_tensor_filter(fa, on));
        } else {
            HIP_TRY(launch_rgba_filter(a, on));
        }
        return H263MI_OK;
    }
    ResizeArgs a{};
    a.src = rz.scratch->pixels.as<uint8_t>();
    a.dst = d_dst;
    a.cols = rz.scratch->spans.as<ResizeSpan>();
    a.rows = a.cols + rz.ow;
    a.w = L.width;
    a.h = L.height;
    a.ow = rz.ow;
    a.oh = rz.oh;
    a.pitch = rz.pitch;
    a.d = L.width * L.height;
    a.inv_d = 1.0f / (float)a.d;
    a.n_pictures = n;
    // a framing: the resize inside the destination rectangle (its span tables, its divisor), the W' x H' output around it
    FrameRect fr{};
    if (rz.framed.on) {
        const h263mi_framing_rects &rc = rz.framed.rc;
        a.rows = a.cols + rc.dst_w;
        a.ow = rc.dst_w;
        a.oh = rc.dst_h;
        a.d = (uint32_t)rc.src_w * rc.src_h;
        a.inv_d = 1.0f / (float)a.d;
        fr.cw = rz.ow, fr.ch = rz.oh, fr.dx = rc.dst_x, fr.dy = rc.dst_y;
        fr.pad = rz.framed.pad;
        fr.keep = rz.framed.keep ? 1u : 0u;
    }
    if (rz.tensor.on) {                        // the same resize, ending in planar float stores (k_tensor_resize)
        TensorArgs ta{};
        ta.r = a;
        for (int c = 0; c < 3; c++) ta.scale[c] = rz.tensor.scale[c], ta.bias[c] = rz.tensor.bias[c];
        ta.dtype = rz.tensor.dtype;
        ta.bgr = rz.tensor.bgr;
        ta.stride_c = rz.tensor.stride_c;
        ta.stride_h = rz.tensor.stride_h;
        if (rz.framed.on) {
            if (!launch_tensor_resize_framed) return H263MI_ERR_HIP;       // (kernels.h: only a stub runtime lacks it)
            RC_TRY(time_begin(3, on));
            HIP_TRY(launch_tensor_resize_framed(FramedTensorArgs{ta, fr}, on));
            return H263MI_OK;
        }
        if (!launch_tensor_resize) return H263MI_ERR_HIP;  // (kernels.h: only a stub runtime lacks it)
        RC_TRY(time_begin(3, on));
        HIP_TRY(launch_tensor_resize(ta, on));
        return H263MI_OK;
    }
    if (rz.framed.on) {
        if (!launch_rgba_resize_framed) return H263MI_ERR_HIP;             // (kernels.h: only a stub runtime lacks it)
        RC_TRY(time_begin(3, on));
        HIP_TRY(launch_rgba_resize_framed(FramedResizeArgs{a, fr}, on));
        return H263MI_OK;
    }
    if (!launch_rgba_resize) return H263MI_ERR_HIP;        // (kernels.h: only a stub runtime lacks it)
    RC_TRY(time_begin(3, on));
    HIP_TRY(launch_rgba_resize(a, on));
    return H263MI_OK;
}

bool h263mi_batch::any_picture() const
{
    for (const StreamState &t : ss)
        if (t.cur >= 0) return true;
    return false;
}

bool h263mi_batch::uniform() const
{
    for (const StreamState &t : ss)
        if (!t.active || t.cur != ss[0].cur || t.has_ref != ss[0].has_ref) return false;
    return true;
}

bool h263mi_batch::pending_uniform() const
{
    for (int8_t v : pending.set)
        if (v != pending.set[0]) return false;
    return true;
}

int h263mi_batch::forget_pictures()
{
    const int rc = flush_pending();        // what was asked to be rendered still is
    for (StreamState &t : ss) {
        const bool active = t.active;
        t = StreamState();
        t.active = active;
    }
    parser_ctx.clear();
    return rc;
}

int h263mi_batch::forget_stream(uint32_t i)
{
    RC_TRY(flush_pending());
    const bool active = ss[i].active;
    ss[i] = StreamState();
    ss[i].active = active;
    if (i < parser_ctx.size()) parser_ctx[i] = bits::ParserContext();
    return H263MI_OK;
}

void h263mi_batch::release_frames()
{
    if (frames[0]) (void)hipFree(frames[0] - frame_skew);         // (one allocation holds both sets)
    frames[0] = frames[1] = nullptr;
}

h263mi_batch::~h263mi_batch()
{
    DeviceGuard g(device);
    (void)hipStreamSynchronize(stream);
    if (trace_host && host_calls)
        fprintf(stderr, "h263mi batch (%u streams): %u host submits; ms per call: parse %.3f, wait for slot %.3f, pack %.3f, "
                        "enqueue %.3f (copies %.3f, launch %.3f)\n", n, host_calls, host_ms[0] / host_calls, host_ms[1] / host_calls,
                host_ms[2] / host_calls, host_ms[3] / host_calls, host_ms[4] / host_calls, host_ms[5] / host_calls);
    pool.reset();                               // the host threads first: nothing of theirs may outlive the staging memory
    release_frames();
    if (post_stream) {
        (void)hipStreamSynchronize(post_stream);
        (void)hipStreamDestroy(post_stream);
    }
    if (ev_recon_done) (void)hipEventDestroy(ev_recon_done);
    for (hipEvent_t e : ev_post_done)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
    // (the staging memory, the rings and the status words go with the members)
}

// =========================================================================================
// launch timing (h263mi_batch_timing_begin / _end).  Consecutive launches of the same kernel form a CHAIN that is
// bracketed by ONE pair of events -- begin in front of the first launch, end behind the last -- and the chain's time
// is shared out over its launches: an event pair around every single launch put a 6 us bubble between two launches
// (2 % of a frame index of the 64-stream bench; tools/probes/timing_overhead.py).  A chain ends where the kernel
// changes and in front of anything else that is queued on the stream (copies, the status read of sync), so only
// launches -- and the gaps between back-to-back launches -- are inside.
// =========================================================================================
int h263mi_batch::time_close()
{
    if (chain_kernel < 0) return H263MI_OK;
    const int k = chain_kernel;
    chain_kernel = -1;
    HIP_TRY(hipEventRecord(ev_pool[ev_used + 1], chain_on));
    ev_ranges.push_back(TimedChain{ev_used, k, chain_launches});
    ev_used += 2;
    return H263MI_OK;
}

int h263mi_batch::time_begin(int kernel_id, hipStream_t on)
{
    if (!timing) return H263MI_OK;
    if (!on) on = stream_of(kernel_id);
    if (chain_kernel == kernel_id && chain_on == on) {
        chain_launches++;
        return H263MI_OK;
    }
    RC_TRY(time_close());
    if (ev_used + 2 > ev_pool.size()) {
        for (int i = 0; i < 2; i++) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e));
            ev_pool.push_back(e);
        }
    }
    HIP_TRY(hipEventRecord(ev_pool[ev_used], on));
    chain_kernel = kernel_id;
    chain_on = on;
    chain_launches = 1;
    return H263MI_OK;
}

// =========================================================================================
// the work
// =========================================================================================
int h263mi_batch::submit(uint8_t picture_type, const MbRecord *d_mbs, const h263mi_coeff_source &src, bool with_post, const uint8_t *types)
{
    if (!with_post) RC_TRY(flush_pending());
    ReconArgs a{};
    a.L = L;
    a.mbs = d_mbs;
    a.coeffs = src.coeffs;
    a.block_first_event = src.first_event;
    a.events = src.events;
    a.n_events = src.n_events ? src.n_events : 0xffffffffu;
    a.mb_group_index = src.group_index;
    a.mb_base = src.mb_base;
    a.groups_per_picture = recon_tiles_x(L) * L.mbh;
    a.coeff_base = src.coeff_base;
    a.status = status.d;
    a.coeff_pool_blocks = src.pool_blocks;
    a.coeff_checked = src.checked ? 1u : 0u;
    a.n_pictures = n;
    a.mbs_per_picture = L.mbw * L.mbh;
    a.tiles_x = recon_tiles_x(L);
    a.tiles_y = recon_tiles_y(L);
    a.frame_set[0] = frames[0];
    a.frame_set[1] = frames[1];
    PostArgs pa{};
    // A pending rendering of planes in a YUV layout: k_frame's post-processing half is the YUV instantiation -- or, when RGBA
    // is pending too, the RGBA goes with k_frame as ever and the planes follow in a k_post_yuv launch of their own
    const bool yuv_post = with_post && pending.yuv.on() && pending.planes;
    const bool yuv_split = yuv_post && (pending.rgba || pending.rgba_ptrs);
    if (with_post) pa = post_args(0, pending.strength.of(0), pending.rgba, yuv_split ? nullptr : pending.planes);
    if (with_post) pa.rgba_ptrs = pending.rgba_ptrs;       // (read in the per-stream branch of the kernel only)
    if (with_post) pa.rgba_scale = pending.out.scale, pa.rgba_pitch = pending.out.pitch;
    // one strength for every picture of the launch, or one per stream (then it travels in the streams' words)
    const bool all_same = uniform() && (!with_post || (pending_uniform() && pending.set[0] >= 0 && !pending.rgba_ptrs &&
                                                       pending.strength.same_for_all()));
    int out0 = 0;
    std::vector<uint32_t> words;                 // one STREAM_* word per stream when they differ (empty: they do not)
    const bool words_inline = n <= STREAM_WORDS_INLINE;       // ... which then travel in the launch's kernel arguments
    if (all_same) {
        const int cur = ss[0].cur;
        out0 = cur < 0 ? 0 : (cur ^ 1);
        // get_reference_picture() hands out the LAST picture whenever a reference exists (state.rs:72-78)
        a.ref = frames[cur < 0 ? 1 : cur];
        a.cur = frames[out0];
        a.has_ref = (ss[0].has_ref && cur >= 0) ? 1u : 0u;
        if (with_post) pa.frames = frames[pending.set[0]];
    } else {
        words.resize(n);
        for (uint32_t i = 0; i < n; i++) {
            const StreamState &t = ss[i];
            uint32_t w = (t.cur != 0 ? STREAM_REF_SET1 : 0u) | ((t.has_ref && t.cur >= 0) ? STREAM_HAS_REF : 0u) |
                         (t.active ? 0u : STREAM_RECON_SKIP);
            if (!with_post || pending.set[i] < 0) w |= STREAM_POST_SKIP;
            else w |= (pending.set[i] == 1 ? STREAM_POST_SET1 : 0u) | ((uint32_t)pending.strength.of(i) << STREAM_STRENGTH_SHIFT);
            words[i] = w;
        }
        // (a batch of more than STREAM_WORDS_INLINE streams: the words go to device memory, a small copy in front of the launch)
        const uint32_t *d_words = nullptr;
        if (!words_inline) RC_TRY(upload(word_ring, words.data(), &d_words, stream));
        a.stream_state = d_words;
        a.ref = frames[0];                   // (never used with per-stream words; never null)
        a.cur = frames[1];
        if (with_post) {
            pa.stream_state = d_words;
            pa.frame_set[0] = frames[0];
            pa.frame_set[1] = frames[1];
            pa.frames = frames[0];
        }
    }
    // the set being overwritten was last read by the post-processing of the picture before the last one
    if (overlap_post) {
        HIP_TRY(hipStreamWaitEvent(stream, ev_post_done[out0], 0));
        if (!all_same) HIP_TRY(hipStreamWaitEvent(stream, ev_post_done[out0 ^ 1], 0));     // (streams write either set)
    }
    if (with_post) {
        RC_TRY(time_begin(2));
        const uint32_t *launch_words = !words.empty() && words_inline ? words.data() : nullptr;
        const bool descending = (frame_launches++ & 1u) != 0;
        hipError_t e;
        if (yuv_post && !yuv_split)
            e = launch_frame_yuv ? launch_frame_yuv(a, pa, pending.yuv.out(pending.planes), stream, descending, launch_words)
                                 : hipErrorUnknown;        // (kernels.h: only a stub runtime lacks it)
        else e = launch_frame(a, pa, stream, descending, launch_words);
        if (e != hipSuccess) {               // the deferred post-processing must not get lost with the failed launch
            (void)flush_pending();
            return map_hip_error(e);
        }
        pending.valid = false;
        if (yuv_split) RC_TRY(launch_post_sets(pending.set, pending.strength, nullptr, pending.planes, stream, nullptr, OutLayout(), &pending.yuv));
        if (pending.resize.on()) {           // the full-size pictures k_frame has just written into the scratch, resized
            const RgbaLayout::Resize rz = std::move(pending.resize);
            pending.resize = RgbaLayout::Resize();
            RC_TRY(launch_resize(rz, pending.set, pending.resize_dst, stream));
        }
        if (pending.yuv.resize.on() && pending.plane_dst) {     // ... and the full-size planes in theirs
            const YuvLayout::Resize rz = std::move(pending.yuv.resize);
            pending.yuv = YuvLayout();
            RC_TRY(launch_plane_resize(rz, pending.set, pending.plane_dst, pending.plane_wide, stream));
        }
    } else {
        RC_TRY(time_begin(0));
        HIP_TRY(launch_recon(a, stream, !words.empty() && words_inline ? words.data() : nullptr));
    }
    if (overlap_post) HIP_TRY(hipEventRecord(ev_recon_done, stream));
    // reference bookkeeping, state.rs:464-483, per stream
    for (uint32_t i = 0; i < n; i++) {
        StreamState &t = ss[i];
        if (!t.active) continue;
        const uint8_t type = types ? types[i] : picture_type;
        t.unsynced++;
        if (type == H263MI_PICTURE_I) t.has_ref = false;
        t.cur = (int8_t)(t.cur < 0 ? 0 : (t.cur ^ 1));
        if (type != H263MI_PICTURE_DISPOSABLE_P) t.has_ref = true;
    }
    return H263MI_OK;
}

PostArgs h263mi_batch::post_args(int set, uint8_t strength, uint8_t *d_rgba, uint8_t *d_planes) const
{
    PostArgs a{};
    a.L = L;
    a.frames = frames[set];
    a.rgba = d_rgba;
    a.planes_out = d_planes;
    a.n_pictures = n;
    a.strength = strength;
    set_post_tiles(a);
    a.luma_only = 0;
    return a;
}

int h263mi_batch::launch_post_sets(const std::vector<int8_t> &sets, const Strengths &strength, uint8_t *d_rgba, uint8_t *d_planes,
                                   hipStream_t on, uint8_t *const *rgba_ptrs, OutLayout out, const YuvLayout *yuv)
{
    if (yuv && yuv->on() && d_planes) {
        // planes in a YUV layout: the RGBA of the call first, by the kernels it always takes, then the planes alone
        if (d_rgba || rgba_ptrs) RC_TRY(launch_post_sets(sets, strength, d_rgba, nullptr, on, rgba_ptrs, out));
        d_rgba = nullptr;
        rgba_ptrs = nullptr;
        out = OutLayout();
    } else {
        yuv = nullptr;
    }
    bool same = rgba_ptrs == nullptr && strength.same_for_all(), any = false;
    for (int8_t v : sets) {
        same = same && v == sets[0];
        any = any || v >= 0;
    }
    if (!any) return H263MI_OK;
    PostArgs a = post_args(sets[0] >= 0 ? sets[0] : 0, strength.of(0), d_rgba, d_planes);
    a.rgba_ptrs = rgba_ptrs;
    a.rgba_scale = out.scale;
    a.rgba_pitch = out.pitch;
    std::vector<uint32_t> words;
    const bool words_inline = n <= STREAM_WORDS_INLINE;
    if (!same) {
        words.resize(n);
        for (uint32_t i = 0; i < n; i++)
            words[i] = STREAM_RECON_SKIP | (sets[i] < 0 ? STREAM_POST_SKIP : (sets[i] == 1 ? STREAM_POST_SET1 : 0u)) |
                       ((uint32_t)strength.of(i) << STREAM_STRENGTH_SHIFT);
        const uint32_t *d_words = nullptr;
        if (!words_inline) RC_TRY(upload(word_ring, words.data(), &d_words, on));
        a.stream_state = d_words;
        a.frame_set[0] = frames[0];
        a.frame_set[1] = frames[1];
    }
    RC_TRY(time_begin(1));
    const uint32_t *launch_words = !words.empty() && words_inline ? words.data() : nullptr;
    if (yuv) {
        if (!launch_post_yuv) return H263MI_ERR_HIP;           // (kernels.h: only a stub runtime lacks it)
        HIP_TRY(launch_post_yuv(a, yuv->out(d_planes), on, launch_words));
    } else {
        HIP_TRY(launch_post(a, on, launch_words));
    }
    return H263MI_OK;
}

int h263mi_batch::note_pending(const Strengths &strength, uint8_t *d_rgba, uint8_t *d_planes, uint8_t *const *host_ptrs)
{
    pending.valid = false;
    pending.rgba_ptrs = nullptr;
    pending.resize = RgbaLayout::Resize();
    pending.yuv = d_planes ? yuv : YuvLayout();      // (captured here, at the request, like the RGBA shape)
    pending.plane_dst = nullptr;
    // a YUV resize: the deferred rendering writes the full-size planes into its scratch, k_plane_resize follows it
    auto note_planes = [&]() -> int {
        if (!pending.yuv.resize.on()) return H263MI_OK;
        RC_TRY(plane_resize_dst(pending.yuv.resize, pending.set, d_planes, stream, &pending.plane_dst, &pending.plane_wide));
        pending.planes = pending.yuv.resize.scratch->pixels.as<uint8_t>();
        return H263MI_OK;
    };
    if (layout.resize.on() && (d_rgba || host_ptrs)) {
        // a resize: the deferred rendering writes the full-size pictures into the scratch, k_rgba_resize follows it (the
        // resize -- scratch, size, destinations -- is captured here, at the request)
        for (uint32_t i = 0; i < n; i++)
            pending.set[i] = (ss[i].active && (!host_ptrs || host_ptrs[i])) ? ss[i].cur : (int8_t)-1;
        RC_TRY(resize_dst(layout, pending.set, d_rgba, host_ptrs, stream, &pending.resize_dst));
        pending.planes = d_planes;
        RC_TRY(note_planes());
        pending.resize = layout.resize;
        pending.out = OutLayout();
        pending.valid = true;
        pending.strength = strength;
        pending.rgba = layout.resize.scratch->pixels.as<uint8_t>();
        return H263MI_OK;
    }
    // (an output layout places each stream's picture through a per-stream pointer; the layout is captured here, at the request)
    std::vector<uint8_t *> placed;
    if (!host_ptrs && layout_ptrs(layout, d_rgba, placed)) host_ptrs = placed.data();
    pending.out = layout.kernel;
    if (host_ptrs) RC_TRY(upload(ptr_ring, host_ptrs, &pending.rgba_ptrs, stream));
    for (uint32_t i = 0; i < n; i++)
        pending.set[i] = (ss[i].active && (!host_ptrs || host_ptrs[i])) ? ss[i].cur : (int8_t)-1;
    pending.planes = d_planes;
    RC_TRY(note_planes());
    pending.valid = d_rgba || d_planes || host_ptrs;
    pending.strength = strength;
    pending.rgba = d_rgba;
    return H263MI_OK;
}

int h263mi_batch::flush_pending()
{
    if (!pending.valid) return H263MI_OK;
    pending.valid = false;
    const RgbaLayout::Resize rz = std::move(pending.resize);
    pending.resize = RgbaLayout::Resize();
    const YuvLayout::Resize yrz = std::move(pending.yuv.resize);
    pending.yuv.resize = YuvLayout::Resize();
    RC_TRY(launch_post_sets(pending.set, pending.strength, pending.rgba, pending.planes, stream, pending.rgba_ptrs, pending.out, &pending.yuv));
    if (rz.on()) RC_TRY(launch_resize(rz, pending.set, pending.resize_dst, stream));
    return yrz.on() && pending.plane_dst ? launch_plane_resize(yrz, pending.set, pending.plane_dst, pending.plane_wide, stream) : H263MI_OK;
}

int h263mi_batch::render(const Strengths &strength, uint8_t *d_rgba, uint8_t *d_planes, bool only_active, uint8_t *const *host_ptrs,
                         const RgbaLayout *rgba_shape, const YuvLayout *yuv_shape)
{
    if (!any_picture()) return H263MI_ERR_NO_PICTURE;
    RC_TRY(flush_pending());
    const RgbaLayout &lay = rgba_shape ? *rgba_shape : layout;
    const YuvLayout &yl = yuv_shape ? *yuv_shape : yuv;
    const RgbaLayout::Resize &rz = lay.resize;
    const bool resized = rz.on() && (d_rgba || host_ptrs);
    std::vector<uint8_t *> placed;
    if (!resized && !host_ptrs && layout_ptrs(lay, d_rgba, placed)) host_ptrs = placed.data();
    std::vector<int8_t> sets(n);
    bool reads[2] = {false, false};
    for (uint32_t i = 0; i < n; i++) {
        sets[i] = ((only_active && !ss[i].active) || (host_ptrs && !host_ptrs[i])) ? (int8_t)-1 : ss[i].cur;
        if (sets[i] >= 0) reads[sets[i]] = true;
    }
    if (overlap_post) HIP_TRY(hipStreamWaitEvent(post_stream, ev_recon_done, 0));
    uint8_t *const *d_out_ptrs = nullptr;
    // a YUV resize: the full-size planes into its scratch (the default kernels), k_plane_resize behind the rendering
    const bool planes_resized = yl.resize.on() && d_planes;
    const PlaneDst *d_plane_dst = nullptr;
    bool plane_wide = false;
    if (planes_resized) {
        RC_TRY(plane_resize_dst(yl.resize, sets, d_planes, stream_of(1), &d_plane_dst, &plane_wide));
        d_planes = yl.resize.scratch->pixels.as<uint8_t>();
    }
    if (resized) {
        // full size into the scratch (the default kernels), then k_rgba_resize right behind it on the same stream
        RC_TRY(resize_dst(lay, sets, d_rgba, host_ptrs, stream_of(1), &d_out_ptrs));
        RC_TRY(launch_post_sets(sets, strength, rz.scratch->pixels.as<uint8_t>(), d_planes, stream_of(1), nullptr, OutLayout(), &yl));
        RC_TRY(launch_resize(rz, sets, d_out_ptrs, stream_of(1)));
    } else {
        if (host_ptrs) RC_TRY(upload(ptr_ring, host_ptrs, &d_out_ptrs, stream_of(1)));
        RC_TRY(launch_post_sets(sets, strength, d_rgba, d_planes, stream_of(1), d_out_ptrs, lay.kernel, &yl));
    }
    if (planes_resized) RC_TRY(launch_plane_resize(yl.resize, sets, d_plane_dst, plane_wide, stream_of(1)));
    // a later reconstruction may overwrite a frame set only when every post-processing that reads it is done: streams
    // that have drifted apart read both sets
    if (overlap_post)
        for (int k = 0; k < 2; k++)
            if (reads[k]) HIP_TRY(hipEventRecord(ev_post_done[k], post_stream));
    return H263MI_OK;
}

int h263mi_batch::sync(int *stream_rc)
{
    RC_TRY(flush_pending());
    RC_TRY(time_close());
    if (overlap_post) HIP_TRY(hipStreamSynchronize(post_stream));
    HIP_TRY(hipMemcpyAsync(status.h, status.d, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    int first_error = H263MI_OK;
    for (uint32_t i = 0; i < n; i++) {
        StreamState &t = ss[i];
        const uint32_t st = status.h[i];
        int rc = H263MI_OK;
        if (st) {
            // A picture the device rejected must not become the stream's last / reference picture.  One picture since
            // the last good sync: the previous frame set is intact, go back to it.  More than one: the set it lived
            // in has been overwritten by the ping-pong, so no picture survives (like a reset of the stream).
            if (t.unsynced <= 1) {
                t.cur = t.good_cur;
                t.has_ref = t.good_has_ref;
            } else {
                t.cur = -1;
                t.has_ref = false;
            }
            rc = (st & STATUS_INTER_WITHOUT_REFERENCE) ? H263MI_ERR_UNCODED_IFRAME_BLOCKS : H263MI_ERR_INVALID_ARGUMENT;
            if (first_error == H263MI_OK) first_error = rc;
        }
        t.good_cur = t.cur;
        t.good_has_ref = t.has_ref;
        t.unsynced = 0;
        if (stream_rc) stream_rc[i] = rc;
    }
    if (first_error != H263MI_OK) HIP_TRY(hipMemsetAsync(status.d, 0, (size_t)n * sizeof(uint32_t), stream));
    return first_error;
}

int h263mi_batch::copy_yuv(uint32_t s, uint8_t *y, uint8_t *cb, uint8_t *cr)
{
    if (s >= n) return H263MI_ERR_INVALID_ARGUMENT;
    if (ss[s].cur < 0) return H263MI_ERR_NO_PICTURE;
    RC_TRY(time_close());
    const uint8_t *f = frames[ss[s].cur] + (size_t)s * L.frame_bytes;
    // DecodedPicture planes are exact-size and tightly packed (picture.rs:39-58)
    if (y) HIP_TRY(hipMemcpy2DAsync(y, L.width, f, L.pitch_y, L.width, L.height, hipMemcpyDeviceToHost, stream));
    if (cb) HIP_TRY(hipMemcpy2DAsync(cb, L.cwidth, f + L.off_cb, L.pitch_c, L.cwidth, L.cheight, hipMemcpyDeviceToHost, stream));
    if (cr) HIP_TRY(hipMemcpy2DAsync(cr, L.cwidth, f + L.off_cr, L.pitch_c, L.cwidth, L.cheight, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return H263MI_OK;
}

int h263mi_batch::digest_yuv(uint32_t seed, uint32_t *digests, int *stream_rc)
{
    if (!digests || !digest_seed_valid(seed)) return H263MI_ERR_INVALID_ARGUMENT;
    RC_TRY(time_close());                        // a digest is not part of any kernel's time
    // DecodedPicture planes are exact-size (picture.rs:39-58): the windows of the pitched planes, where they are
    digest_planes.clear();
    bool missing = false;
    for (uint32_t i = 0; i < n; i++) {
        if (ss[i].cur < 0) {
            missing = true;
            continue;
        }
        const uint64_t f = (uint64_t)(frames[ss[i].cur] - frames[0]) + (uint64_t)i * L.frame_bytes;
        digest_planes.push_back(h263mi_digest_span{f, L.pitch_y, L.width, L.height, i, 0});
        digest_planes.push_back(h263mi_digest_span{f + L.off_cb, L.pitch_c, L.cwidth, L.cheight, i, 0});
        digest_planes.push_back(h263mi_digest_span{f + L.off_cr, L.pitch_c, L.cwidth, L.cheight, i, 0});
    }
    if (!digest_planes.empty())
        RC_TRY(digest_spans(digest_words, placement, frames[0], 2ull * n * L.frame_bytes, digest_planes.data(),
                            (uint32_t)digest_planes.size(), seed, digests, n, stream));
    for (uint32_t i = 0; i < n; i++) {
        if (ss[i].cur < 0) digests[i] = 0;
        if (stream_rc) stream_rc[i] = ss[i].cur < 0 ? H263MI_ERR_NO_PICTURE : H263MI_OK;
    }
    return missing && !stream_rc ? H263MI_ERR_NO_PICTURE : H263MI_OK;
}

namespace h263mi {

int digest_spans(PinnedPair<uint64_t> &buf, const HostPlacement &where, const uint8_t *d_base, uint64_t buffer_bytes,
                 const h263mi_digest_span *spans, uint32_t n_spans, uint32_t seed, uint32_t *digests, uint32_t n_digests,
                 hipStream_t stream)
{
    if (!digests || !digest_table(spans, n_spans, n_digests, buffer_bytes, d_base != nullptr, seed, nullptr, nullptr, nullptr))
        return H263MI_ERR_INVALID_ARGUMENT;
    if (!launch_digest) return H263MI_ERR_HIP;             // (kernels.h: only a stub runtime lacks it)
    // one buffer, in 64-bit words: [the spans][A, B per digest][the digests, two to a word]
    static_assert(sizeof(DigestSpan) % 8 == 0, "the span table is addressed in 64-bit words");
    const size_t w_spans = (size_t)n_spans * (sizeof(DigestSpan) / 8), w_acc = 2 * (size_t)n_digests, w_out = ((size_t)n_digests + 1) / 2;
    RC_TRY(buf.reserve(w_spans + w_acc + w_out, 0, where));
    DigestArgs a{};
    digest_table(spans, n_spans, n_digests, buffer_bytes, d_base != nullptr, seed, reinterpret_cast<DigestSpan *>(buf.h),
                 reinterpret_cast<unsigned long long *>(buf.h + w_spans), &a.n_items);
    a.base = d_base;
    a.spans = reinterpret_cast<const DigestSpan *>(buf.d);
    a.acc = reinterpret_cast<unsigned long long *>(buf.d + w_spans);
    a.n_spans = n_spans;
    DigestFinalArgs f{};
    f.acc = a.acc;
    f.out = reinterpret_cast<uint32_t *>(buf.d + w_spans + w_acc);
    f.n_digests = n_digests;
    HIP_TRY(hipMemcpyAsync(buf.d, buf.h, (w_spans + w_acc) * 8, hipMemcpyHostToDevice, stream));
    HIP_TRY(launch_digest(a, f, stream));
    HIP_TRY(hipMemcpyAsync(buf.h + w_spans + w_acc, f.out, (size_t)n_digests * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    memcpy(digests, buf.h + w_spans + w_acc, (size_t)n_digests * 4);
    return H263MI_OK;
}

int make_strengths(uint8_t strength, const uint8_t *strengths, uint32_t n, bool from_header_allowed, h263mi_batch::Strengths &out)
{
    out = h263mi_batch::Strengths();
    if (strengths) {
        out.per_stream.assign(strengths, strengths + n);
        for (uint8_t v : out.per_stream)
            if (v > 12) return H263MI_ERR_INVALID_ARGUMENT;
        return H263MI_OK;
    }
    if (strength == H263MI_STRENGTH_FROM_HEADER) {
        if (!from_header_allowed) return H263MI_ERR_INVALID_ARGUMENT;
        out.per_stream.assign(n, 0);             // (filled in per picture by the entry that has parsed the headers)
        return H263MI_OK;
    }
    if (strength > 12) return H263MI_ERR_INVALID_ARGUMENT;
    out.uniform = strength;
    return H263MI_OK;
}

// Where the host side of device `dev` belongs: the PCI addresses of the visible devices -> worker_pool.cpp (sysfs)
HostPlacement placement_of_device(int dev)
{
    // looked up once per (device, ranks per node, switches): a mixed-size set makes a batch whenever a class is made or
    // rebuilt -- out of untrusted bitstreams -- and the look-up reads a few hundred sysfs files
    static std::mutex cache_mutex;
    static std::map<std::string, HostPlacement> cache;
    const uint32_t ranks = host_thread_plan(1, 0).ranks;
    std::string key = std::to_string(dev) + "|" + std::to_string(ranks);
    for (const char *name : {"H263MI_NUMA", "H263MI_NUMA_NODE", "H263MI_SYSFS_ROOT"}) {
        const char *v = getenv(name);
        key += std::string("|") + (v ? v : "");
    }
    {
        std::lock_guard<std::mutex> l(cache_mutex);
        auto it = cache.find(key);
        if (it != cache.end()) return it->second;
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return HostPlacement();
    std::vector<std::string> ids((size_t)count);
    for (int d = 0; d < count; d++) {
        char id[64] = {0};
        if (hipDeviceGetPCIBusId(id, (int)sizeof id, d) == hipSuccess) ids[(size_t)d] = id;
        else (void)hipGetLastError();
    }
    const HostPlacement p = host_placement(ids, dev, ranks);
    std::lock_guard<std::mutex> l(cache_mutex);
    cache[key] = p;
    return p;
}

int batch_create(uint32_t n_streams, uint32_t w, uint32_t h, const h263mi_backend_cfg *cfg, h263mi_batch **out)
{
    if (!out || !n_streams || !w || !h) return H263MI_ERR_INVALID_ARGUMENT;
    if (!layout_fits(w, h)) return H263MI_ERR_PICTURE_FORMAT_INVALID;        // before anything is allocated
    const int dev = cfg ? cfg->device_id : 0;
    RC_TRY(check_device(dev));
    DeviceGuard g(dev);
    if (!g.ok) return H263MI_ERR_NO_DEVICE;
    h263mi_batch *b = new (std::nothrow) h263mi_batch();
    if (!b) return H263MI_ERR_OUT_OF_MEMORY;
    b->device = dev;
    b->stream = cfg ? (hipStream_t)cfg->stream : nullptr;
    int rc = H263MI_OK;
    b->pipeline_post = cfg && (cfg->flags & H263MI_CFG_PIPELINE_POST);
    b->trusted_arrays = cfg && (cfg->flags & H263MI_CFG_TRUSTED_ARRAYS);
    b->placement = placement_of_device(dev);
    if (cfg && (cfg->flags & H263MI_CFG_OVERLAP_POST) && !b->pipeline_post) {
        b->overlap_post = true;
        if (fault_now() || hipStreamCreateWithFlags(&b->post_stream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&b->ev_recon_done, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&b->ev_post_done[0], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&b->ev_post_done[1], hipEventDisableTiming) != hipSuccess)
            rc = H263MI_ERR_HIP;
    }
    if (rc == H263MI_OK) rc = b->alloc(n_streams, w, h);
    if (rc != H263MI_OK) {
        delete b;
        return rc;
    }
    *out = b;
    return H263MI_OK;
}

// The allocation a device pointer of the caller lies in bounds what may be read through it: `bytes` receives what is left
// of it from `p` on.  H263MI_ERR_INVALID_ARGUMENT when the runtime does not know the pointer (then the caller must say how
// large its arrays are, or vouch for them: H263MI_CFG_TRUSTED_ARRAYS).
static int bytes_behind(const void *p, size_t *bytes)
{
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (fault_now()) return H263MI_ERR_OUT_OF_MEMORY;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)const_cast<void *>(p)) != hipSuccess || !base) {
        (void)hipGetLastError();
        return H263MI_ERR_INVALID_ARGUMENT;
    }
    const size_t off = (size_t)((const uint8_t *)p - (const uint8_t *)base);
    if (off > size) return H263MI_ERR_INVALID_ARGUMENT;
    *bytes = size - off;
    return H263MI_OK;
}

// The caller's device arrays of h263mi_batch_submit / _decode / _decode_events -> what the waves may read (ABI 7: checked
// unless the batch was made with H263MI_CFG_TRUSTED_ARRAYS).  Counts the caller gave are taken as they are; what it did not
// say is bounded by the allocation the pointer lies in, so that no record, offset or event of its arrays -- whatever they
// hold -- can take a wave outside memory the caller owns.  The fixed-size arrays (records, bases) must fit theirs.
static int bound_device_arrays(const h263mi_batch *b, const h263mi_mb_record *d_mbs, uint64_t coeff_pool_blocks, uint64_t n_events,
                               h263mi_coeff_source &src)
{
    src.pool_blocks = coeff_pool_blocks;
    src.n_events = (uint32_t)n_events;
    if (b->trusted_arrays) {
        src.checked = coeff_pool_blocks != 0;
        return H263MI_OK;
    }
    size_t left = 0;
    RC_TRY(bytes_behind(d_mbs, &left));
    if (left < (size_t)b->n * b->L.mbw * b->L.mbh * sizeof(MbRecord)) return H263MI_ERR_INVALID_ARGUMENT;
    if (src.coeff_base) {
        RC_TRY(bytes_behind(src.coeff_base, &left));
        if (left < (size_t)b->n * sizeof(uint64_t)) return H263MI_ERR_INVALID_ARGUMENT;
    }
    if (src.events) {
        // coded block k of the pool reads first_event[k] and [k + 1]: the offsets array bounds the pool
        RC_TRY(bytes_behind(src.first_event, &left));
        const uint64_t blocks_max = left / sizeof(uint32_t) ? left / sizeof(uint32_t) - 1 : 0;
        if (!coeff_pool_blocks) src.pool_blocks = blocks_max;
        else if (coeff_pool_blocks > blocks_max) return H263MI_ERR_INVALID_ARGUMENT;
        RC_TRY(bytes_behind(src.events, &left));
        const uint64_t words_max = std::min<uint64_t>(left / sizeof(uint32_t), kMaxEventWords);
        if (!n_events) src.n_events = (uint32_t)words_max;
        else if (n_events > words_max) return H263MI_ERR_INVALID_ARGUMENT;
        if (!src.n_events || !src.pool_blocks) return H263MI_ERR_INVALID_ARGUMENT;
    } else if (src.coeffs) {
        RC_TRY(bytes_behind(src.coeffs, &left));
        const uint64_t blocks_max = left / 128;
        if (!coeff_pool_blocks) src.pool_blocks = blocks_max;
        else if (coeff_pool_blocks > blocks_max) return H263MI_ERR_INVALID_ARGUMENT;
        if (!src.pool_blocks) return H263MI_ERR_INVALID_ARGUMENT;
    } else {
        src.pool_blocks = 0;                     // no pool at all: every coded block is outside it
    }
    src.checked = true;
    return H263MI_OK;
}

// The caller's OUTPUT buffers of the same entry points: where the runtime knows the allocation a pointer lies in, it must hold
// what the launch will write (n pictures of RGBA / of filtered planes); a pointer it does not know (the device view of
// registered host memory, another runtime's memory) is taken as it is.  Checked batches only.
static int bound_output_buffers(const h263mi_batch *b, const uint8_t *d_rgba, const uint8_t *d_deblocked)
{
    // (a tensor's base holds whole elements, on a trusted batch too: the kernel stores them as such)
    if (d_rgba && (uintptr_t)d_rgba % b->layout.base_align()) return H263MI_ERR_INVALID_ARGUMENT;
    if (b->trusted_arrays) return H263MI_OK;
    const size_t rgba_bytes = b->layout.bytes;      // (n * w*h*4 unless the batch has an output layout)
    // (n tightly packed I420 pictures unless the batch has a YUV layout or resize)
    const size_t plane_bytes = b->yuv.shaped() ? (size_t)b->yuv.bytes
                                           : (size_t)b->n * ((size_t)b->L.width * b->L.height + 2 * (size_t)b->L.cwidth * b->L.cheight);
    size_t left = 0;
    if (d_rgba) {
        const int rc = bytes_behind(d_rgba, &left);
        if (rc == H263MI_ERR_OUT_OF_MEMORY || (rc == H263MI_OK && left < rgba_bytes)) return rc == H263MI_OK ? H263MI_ERR_INVALID_ARGUMENT : rc;
    }
    if (d_deblocked) {
        const int rc = bytes_behind(d_deblocked, &left);
        if (rc == H263MI_ERR_OUT_OF_MEMORY || (rc == H263MI_OK && left < plane_bytes)) return rc == H263MI_OK ? H263MI_ERR_INVALID_ARGUMENT : rc;
    }
    return H263MI_OK;
}

}  // namespace h263mi

// =========================================================================================
// C ABI: batches over device records
// =========================================================================================
extern "C" {

int h263mi_batch_create(uint32_t n_streams, uint16_t width, uint16_t height, const h263mi_backend_cfg *cfg,
                        h263mi_batch **out)
{
    return batch_create(n_streams, width, height, cfg, out);
}

void h263mi_batch_destroy(h263mi_batch *b) { delete b; }

uint32_t h263mi_batch_mbs_per_picture(const h263mi_batch *b) { return b ? b->L.mbw * b->L.mbh : 0; }

int h263mi_batch_submit(h263mi_batch *b, uint8_t picture_type, const h263mi_mb_record *d_mbs, const int16_t *d_coeffs,
                        const uint64_t *d_coeff_base)
{
    if (!b || !d_mbs || picture_type > H263MI_PICTURE_RESERVED) return H263MI_ERR_INVALID_ARGUMENT;
    DeviceGuard g(b->device);
    h263mi_coeff_source src;
    src.coeffs = d_coeffs;
    src.coeff_base = d_coeff_base;
    RC_TRY(bound_device_arrays(b, d_mbs, 0, 0, src));       // (no size argument here: the pool is bounded by its allocation)
    return b->submit(picture_type, d_mbs, src);
}

// decode + post-process in one call: the common tail of h263mi_batch_decode[_events][_ps]
static int batch_decode_device(h263mi_batch *b, uint8_t picture_type, const h263mi_mb_record *d_mbs, const h263mi_coeff_source &src,
                               const h263mi_batch::Strengths &st, uint8_t *d_rgba, uint8_t *d_deblocked)
{
    if (b->pipeline_post) {
        // this picture's reconstruction and the previous picture's post-processing in one launch; this picture's
        // post-processing waits for the next call (or the next sync)
        RC_TRY(b->submit(picture_type, d_mbs, src, /*with_post=*/b->pending.valid));
        return b->note_pending(st, d_rgba, d_deblocked);
    }
    RC_TRY(b->submit(picture_type, d_mbs, src));
    if (!d_rgba && !d_deblocked) return H263MI_OK;
    return b->render(st, d_rgba, d_deblocked, /*only_active=*/true);
}

int h263mi_batch_decode_ps(h263mi_batch *b, uint8_t picture_type, const h263mi_mb_record *d_mbs, const int16_t *d_coeffs,
                           const uint64_t *d_coeff_base, uint64_t coeff_pool_blocks, uint8_t strength, const uint8_t *strengths,
                           uint8_t *d_rgba, uint8_t *d_deblocked)
{
    if (!b || !d_mbs || picture_type > H263MI_PICTURE_RESERVED) return H263MI_ERR_INVALID_ARGUMENT;
    h263mi_batch::Strengths st;
    RC_TRY(make_strengths(strength, strengths, b->n, /*from_header_allowed=*/false, st));
    DeviceGuard g(b->device);
    h263mi_coeff_source src;
    src.coeffs = d_coeffs;
    src.coeff_base = d_coeff_base;
    RC_TRY(bound_device_arrays(b, d_mbs, coeff_pool_blocks, 0, src));
    RC_TRY(bound_output_buffers(b, d_rgba, d_deblocked));
    return batch_decode_device(b, picture_type, d_mbs, src, st, d_rgba, d_deblocked);
}

int h263mi_batch_decode(h263mi_batch *b, uint8_t picture_type, const h263mi_mb_record *d_mbs, const int16_t *d_coeffs,
                        const uint64_t *d_coeff_base, uint64_t coeff_pool_blocks, uint8_t strength, uint8_t *d_rgba,
                        uint8_t *d_deblocked)
{
    return h263mi_batch_decode_ps(b, picture_type, d_mbs, d_coeffs, d_coeff_base, coeff_pool_blocks, strength, nullptr, d_rgba, d_deblocked);
}

/* the same with the coefficients as sparse events already in device memory (what the host entry points copy there) */
int h263mi_batch_decode_events_ps(h263mi_batch *b, uint8_t picture_type, const h263mi_mb_record *d_mbs,
                                  const uint32_t *d_block_first_event, const uint32_t *d_events, const uint64_t *d_coeff_base,
                                  uint64_t coeff_pool_blocks, uint64_t n_events, uint8_t strength, const uint8_t *strengths,
                                  uint8_t *d_rgba, uint8_t *d_deblocked)
{
    if (!b || !d_mbs || !d_block_first_event || !d_events || picture_type > H263MI_PICTURE_RESERVED || n_events > kMaxEventWords)
        return H263MI_ERR_INVALID_ARGUMENT;
    h263mi_batch::Strengths st;
    RC_TRY(make_strengths(strength, strengths, b->n, /*from_header_allowed=*/false, st));
    DeviceGuard g(b->device);
    h263mi_coeff_source src;
    src.first_event = d_block_first_event;
    src.events = d_events;
    src.coeff_base = d_coeff_base;
    RC_TRY(bound_device_arrays(b, d_mbs, coeff_pool_blocks, n_events, src));
    RC_TRY(bound_output_buffers(b, d_rgba, d_deblocked));
    return batch_decode_device(b, picture_type, d_mbs, src, st, d_rgba, d_deblocked);
}

int h263mi_batch_decode_events(h263mi_batch *b, uint8_t picture_type, const h263mi_mb_record *d_mbs,
                               const uint32_t *d_block_first_event, const uint32_t *d_events, const uint64_t *d_coeff_base,
                               uint64_t coeff_pool_blocks, uint64_t n_events, uint8_t strength, uint8_t *d_rgba,
                               uint8_t *d_deblocked)
{
    return h263mi_batch_decode_events_ps(b, picture_type, d_mbs, d_block_first_event, d_events, d_coeff_base, coeff_pool_blocks, n_events,
                                         strength, nullptr, d_rgba, d_deblocked);
}

int h263mi_batch_render_rgba_ps(h263mi_batch *b, uint8_t strength, const uint8_t *strengths, uint8_t *d_rgba, uint8_t *d_deblocked)
{
    if (!b || (!d_rgba && !d_deblocked)) return H263MI_ERR_INVALID_ARGUMENT;
    h263mi_batch::Strengths st;
    RC_TRY(make_strengths(strength, strengths, b->n, /*from_header_allowed=*/false, st));
    DeviceGuard g(b->device);
    RC_TRY(bound_output_buffers(b, d_rgba, d_deblocked));
    return b->render(st, d_rgba, d_deblocked);
}

int h263mi_batch_set_rgba_layout(h263mi_batch *b, const h263mi_rgba_layout *layout)
{
    if (!b) return H263MI_ERR_INVALID_ARGUMENT;
    h263mi_batch::RgbaLayout lay;
    RC_TRY(make_rgba_layout_shape(b->n, b->L.width, b->L.height, layout, lay));
    DeviceGuard g(b->device);                  // (a resize it replaces frees its scratch)
    b->layout = std::move(lay);
    return H263MI_OK;
}

int h263mi_batch_set_yuv_layout(h263mi_batch *b, const h263mi_yuv_layout *layout)
{
    if (!b) return H263MI_ERR_INVALID_ARGUMENT;
    h263mi_batch::YuvLayout lay;
    RC_TRY(make_yuv_shape(b->device, b->n, b->L.width, b->L.height, layout, lay));
    DeviceGuard g(b->device);                  // (the layout it replaces frees its offsets, unless a pending rendering holds them)
    b->yuv = std::move(lay);
    return H263MI_OK;
}

int h263mi_batch_set_yuv_resize(h263mi_batch *b, const h263mi_yuv_resize *r)
{
    if (!b) return H263MI_ERR_INVALID_ARGUMENT;
    h263mi_batch::YuvLayout shape;
    RC_TRY(make_yuv_resize_shape(b->device, b->n, b->L.width, b->L.height, r, shape));
    DeviceGuard g(b->device);                  // (the shape it replaces frees its memory, unless a pending rendering holds it)
    b->yuv = std::move(shape);
    return H263MI_OK;
}

int h263mi_batch_set_yuv_resize_filtered(h263mi_batch *b, const h263mi_yuv_resize *r, const h263mi_filter *filter)
{
    if (!b) return H263MI_ERR_INVALID_ARGUMENT;
    h263mi_batch::YuvLayout shape;
    RC_TRY(make_yuv_resize_shape(b->device, b->n, b->L.width, b->L.height, r, shape, filter));
    DeviceGuard g(b->device);                  // (the shape it replaces frees its memory, unless a pending rendering holds it)
    b->yuv = std::move(shape);
    return H263MI_OK;
}

int h263mi_batch_set_rgba_resize(h263mi_batch *b, const h263mi_rgba_resize *r)
{
    if (!b) return H263MI_ERR_INVALID_ARGUMENT;
    h263mi_batch::RgbaLayout lay;
    RC_TRY(make_output_shape(b->device, b->n, b->L.width, b->L.height, r, lay));
    DeviceGuard g(b->device);
    b->layout = std::move(lay);
    return H263MI_OK;
}

int h263mi_batch_set_tensor_output(h263mi_batch *b, const h263mi_tensor_out *t)
{
    if (!b) return H263MI_ERR_INVALID_ARGUMENT;
    h263mi_batch::RgbaLayout lay;
    RC_TRY(make_tensor_shape(b->device, b->n, b->L.width, b->L.height, t, lay));
    DeviceGuard g(b->device);                  // (a shape it replaces frees its scratch, unless a pending rendering holds it)
    b->layout = std::move(lay);
    return H263MI_OK;
}

int h263mi_batch_set_rgba_resize_framed(h263mi_batch *b, const h263mi_rgba_resize *r, const h263mi_framing *f)
{
    if (!b) return H263MI_ERR_INVALID_ARGUMENT;
    h263mi_batch::RgbaLayout lay;
    RC_TRY(make_output_shape(b->device, b->n, b->L.width, b->L.height, r, lay, f));
    DeviceGuard g(b->device);                  // (a shape it replaces frees its scratch, unless a pending rendering holds it)
    b->layout = std::move(lay);
    return H263MI_OK;
}

int h263mi_batch_set_tensor_output_framed(h263mi_batch *b, const h263mi_tensor_out *t, const h263mi_framing *f)
{
    if (!b) return H263MI_ERR_INVALID_ARGUMENT;
    h263mi_batch::RgbaLayout lay;
    RC_TRY(make_tensor_shape(b->device, b->n, b->L.width, b->L.height, t, lay, f));
    DeviceGuard g(b->device);
    b->layout = std::move(lay);
    return H263MI_OK;
}

int h263mi_batch_set_rgba_resize_filtered(h263mi_batch *b, const h263mi_rgba_resize *r, const h263mi_framing *f, const h263mi_filter *filter)
{
    if (!b) return H263MI_ERR_INVALID_ARGUMENT;
    h263mi_batch::RgbaLayout lay;
    RC_TRY(make_output_shape(b->device, b->n, b->L.width, b->L.height, r, lay, f, filter));
    DeviceGuard g(b->device);                  // (a shape it replaces frees its scratch, unless a pending rendering holds it)
    b->layout = std::move(lay);
    return H263MI_OK;
}

int h263mi_batch_set_tensor_output_filtered(h263mi_batch *b, const h263mi_tensor_out *t, const h263mi_framing *f, const h263mi_filter *filter)
{
    if (!b) return H263MI_ERR_INVALID_ARGUMENT;
    h263mi_batch::RgbaLayout lay;
    RC_TRY(make_tensor_shape(b->device, b->n, b->L.width, b->L.height, t, lay, f, filter));
    DeviceGuard g(b->device);
    b->layout = std::move(lay);
    return H263MI_OK;
}

int h263mi_batch_render_rgba(h263mi_batch *b, uint8_t strength, uint8_t *d_rgba, uint8_t *d_deblocked)
{
    return h263mi_batch_render_rgba_ps(b, strength, nullptr, d_rgba, d_deblocked);
}

int h263mi_batch_sync(h263mi_batch *b)
{
    if (!b) return H263MI_ERR_INVALID_ARGUMENT;
    DeviceGuard g(b->device);
    return b->sync();
}

int h263mi_batch_reset(h263mi_batch *b)
{
    if (!b) return H263MI_ERR_INVALID_ARGUMENT;
    DeviceGuard g(b->device);                    // (a deferred post-processing may be launched: on the batch's device)
    if (!g.ok) return H263MI_ERR_NO_DEVICE;
    return b->forget_pictures();
}

int h263mi_batch_reset_stream(h263mi_batch *b, uint32_t stream)
{
    if (!b || stream >= b->n) return H263MI_ERR_INVALID_ARGUMENT;
    DeviceGuard g(b->device);
    if (!g.ok) return H263MI_ERR_NO_DEVICE;
    return b->forget_stream(stream);
}

int h263mi_batch_set_active(h263mi_batch *b, const uint8_t *active)
{
    if (!b) return H263MI_ERR_INVALID_ARGUMENT;
    for (uint32_t i = 0; i < b->n; i++) b->ss[i].active = active ? active[i] != 0 : true;
    return H263MI_OK;
}

int h263mi_batch_sync_streams(h263mi_batch *b, int *stream_rc)
{
    if (!b) return H263MI_ERR_INVALID_ARGUMENT;
    DeviceGuard g(b->device);
    return b->sync(stream_rc);
}

int h263mi_batch_stream_has_picture(const h263mi_batch *b, uint32_t stream)
{
    return b && stream < b->n && b->ss[stream].cur >= 0 ? 1 : 0;
}

int h263mi_batch_copy_yuv(h263mi_batch *b, uint32_t stream, uint8_t *y, uint8_t *cb, uint8_t *cr)
{
    if (!b) return H263MI_ERR_INVALID_ARGUMENT;
    DeviceGuard g(b->device);
    return b->copy_yuv(stream, y, cb, cr);
}

int h263mi_batch_digest_yuv(h263mi_batch *b, uint32_t seed, uint32_t *digests, int *stream_rc)
{
    if (!b) return H263MI_ERR_INVALID_ARGUMENT;
    DeviceGuard g(b->device);
    return digest_rc(b->digest_yuv(seed, digests, stream_rc));
}

// the staging of h263mi_adler32_spans_on: per host thread and device, and it only grows (as the scratch of h263mi_deblock)
struct DigestScratch {
    int device = -1;
    PinnedPair<uint64_t> words;
};
static thread_local DigestScratch tls_digest;

int h263mi_adler32_spans_on(const h263mi_backend_cfg *cfg, const uint8_t *d_base, uint64_t buffer_bytes, const h263mi_digest_span *spans,
                            uint32_t n_spans, uint32_t seed, uint32_t *digests, uint32_t n_digests)
{
    if (!digests || !digest_table(spans, n_spans, n_digests, buffer_bytes, d_base != nullptr, seed, nullptr, nullptr, nullptr))
        return H263MI_ERR_INVALID_ARGUMENT;
    const int dev = cfg ? cfg->device_id : 0;
    RC_TRY(check_device(dev));
    DeviceGuard g(dev);
    if (tls_digest.device != dev) {
        tls_digest.words.release();
        tls_digest.device = dev;
    }
    return digest_rc(digest_spans(tls_digest.words, HostPlacement(), d_base, buffer_bytes, spans, n_spans, seed, digests, n_digests,
                                  cfg ? (hipStream_t)cfg->stream : nullptr));
}

int h263mi_batch_adler32_spans(h263mi_batch *b, const uint8_t *d_base, uint64_t buffer_bytes, const h263mi_digest_span *spans,
                               uint32_t n_spans, uint32_t seed, uint32_t *digests, uint32_t n_digests)
{
    if (!b || !digests || !digest_table(spans, n_spans, n_digests, buffer_bytes, d_base != nullptr, seed, nullptr, nullptr, nullptr))
        return H263MI_ERR_INVALID_ARGUMENT;
    DeviceGuard g(b->device);
    RC_TRY(digest_rc(b->sync()));                // (the deferred rendering of a pipelined batch, the second stream of an overlapped one)
    return digest_rc(digest_spans(b->digest_words, b->placement, d_base, buffer_bytes, spans, n_spans, seed, digests, n_digests, b->stream));
}

// h263mi_roi_tensor_on's arguments, decided on the host in the order include/h263mi.h lists; *out: the launch they come to.
// The table itself is never read here: a wave validates its own record (roi_kernel.inl).
static int roi_tensor_args(const uint8_t *d_rgba, uint64_t rgba_bytes, uint32_t n_pictures, uint32_t width, uint32_t height,
                           const h263mi_roi *d_rois, uint32_t n_rois, const h263mi_tensor_out *t, void *d_out, uint64_t out_bytes,
                           uint32_t *d_status, RoiArgs *out)
{
    static_assert(sizeof(h263mi_roi) == 16 && sizeof(RoiRecord) == 16, "a wave reads its record as four words");
    h263mi_batch::RgbaLayout::Resize::Tensor tn;
    uint64_t extent = 0, stride_n = 0;
    RC_TRY(tensor_extent(n_rois ? n_rois : 1, t, &extent, &tn, &stride_n));
    if (!n_pictures || !width || !height || width > 65535 || height > 65535) return H263MI_ERR_INVALID_ARGUMENT;
    if ((uint64_t)width * height >= (1ull << 30)) return H263MI_ERR_INVALID_ARGUMENT;
    if (n_rois > 65535) return H263MI_ERR_INVALID_ARGUMENT;
    if (n_rois && (!d_rgba || !d_rois || !d_out)) return H263MI_ERR_INVALID_ARGUMENT;
    if ((uintptr_t)d_rgba % 16 || (uintptr_t)d_out % tn.elt) return H263MI_ERR_INVALID_ARGUMENT;
    if (rgba_bytes / ((uint64_t)width * height * 4) < n_pictures) return H263MI_ERR_INVALID_ARGUMENT;     // (the product may not fit)
    if (n_rois && out_bytes < extent) return H263MI_ERR_INVALID_ARGUMENT;
    RoiArgs a{};
    a.t.r.src = d_rgba;
    a.t.r.w = width, a.t.r.h = height;
    a.t.r.ow = t->out_width, a.t.r.oh = t->out_height;
    a.t.r.n_pictures = n_pictures;
    for (int c = 0; c < 3; c++) a.t.scale[c] = tn.scale[c], a.t.bias[c] = tn.bias[c];
    a.t.dtype = tn.dtype;
    a.t.bgr = tn.bgr;
    a.t.stride_c = tn.stride_c, a.t.stride_h = tn.stride_h;
    a.rois = reinterpret_cast<const RoiRecord *>(d_rois);
    a.dst = static_cast<uint8_t *>(d_out);
    a.stride_n = stride_n;
    a.status = d_status;
    a.n_rois = n_rois;
    a.inv_ow = 1.0f / (float)a.t.r.ow, a.inv_oh = 1.0f / (float)a.t.r.oh;
    *out = a;
    return H263MI_OK;
}

static int roi_tensor_launch(const RoiArgs &a, hipStream_t stream)
{
    if (!launch_roi_tensor) return H263MI_ERR_HIP;         // (kernels.h: only a stub runtime lacks it)
    auto queue = [&]() -> int {
        HIP_TRY(launch_roi_tensor(a, stream));
        return H263MI_OK;
    };
    return digest_rc(queue());                             // (the call allocates nothing: whatever the runtime refuses is H263MI_ERR_HIP)
}

int h263mi_roi_tensor_on(const h263mi_backend_cfg *cfg, const uint8_t *d_rgba, uint64_t rgba_bytes, uint32_t n_pictures, uint16_t width,
                         uint16_t height, const h263mi_roi *d_rois, uint32_t n_rois, const h263mi_tensor_out *t, void *d_out,
                         uint64_t out_bytes, uint32_t *d_status)
{
    RoiArgs a;
    RC_TRY(roi_tensor_args(d_rgba, rgba_bytes, n_pictures, width, height, d_rois, n_rois, t, d_out, out_bytes, d_status, &a));
    if (!n_rois) return H263MI_OK;
    const int dev = cfg ? cfg->device_id : 0;
    RC_TRY(check_device(dev));
    DeviceGuard g(dev);
    if (!g.ok) return H263MI_ERR_NO_DEVICE;
    return roi_tensor_launch(a, cfg ? (hipStream_t)cfg->stream : nullptr);
}

int h263mi_batch_roi_tensor(h263mi_batch *b, const uint8_t *d_rgba, uint64_t rgba_bytes, const h263mi_roi *d_rois, uint32_t n_rois,
                            const h263mi_tensor_out *t, void *d_out, uint64_t out_bytes, uint32_t *d_status)
{
    if (!b) return H263MI_ERR_INVALID_ARGUMENT;
    RoiArgs a;
    RC_TRY(roi_tensor_args(d_rgba, rgba_bytes, b->n, b->L.width, b->L.height, d_rois, n_rois, t, d_out, out_bytes, d_status, &a));
    DeviceGuard g(b->device);
    RC_TRY(b->sync());                           // (the deferred rendering of a pipelined batch, the second stream of an overlapped one)
    if (!n_rois) return H263MI_OK;
    return roi_tensor_launch(a, b->stream);
}

// =========================================================================================
// change maps (change_kernel.inl)
// =========================================================================================
int h263mi_change_extent(uint32_t n_pictures, uint32_t width, uint32_t height, const h263mi_change *c, uint32_t *gw, uint32_t *gh,
                         uint64_t *cells_bytes)
{
    static_assert(sizeof(h263mi_change) == 16 && sizeof(h263mi_plane_set) == 32, "the structures are part of the ABI");
    if (!c || c->reserved[0] || c->reserved[1] || c->reserved2 || c->cell_log2 < 3 || c->cell_log2 > 6 || c->roll > 1)
        return H263MI_ERR_INVALID_ARGUMENT;
    if (!width || !height || width > 65535 || height > 65535 || (uint64_t)width * height >= (1ull << 30)) return H263MI_ERR_INVALID_ARGUMENT;
    if (n_pictures > CHANGE_MAX_PICTURES) return H263MI_ERR_INVALID_ARGUMENT;
    const uint32_t w = ((width - 1u) >> c->cell_log2) + 1u, h = ((height - 1u) >> c->cell_log2) + 1u;
    if (gw) *gw = w;
    if (gh) *gh = h;
    if (cells_bytes) *cells_bytes = (uint64_t)n_pictures * w * h * 4u;        // (below 2^16 * 2^24 * 4)
    return H263MI_OK;
}

// the bytes from a set's base to behind the last byte of its n pictures; false: the sum wraps
static bool plane_set_end(const h263mi_plane_set &s, uint32_t n, uint32_t w, uint32_t h, uint64_t *end)
{
    uint64_t a, b;
    if (__builtin_mul_overflow((uint64_t)(n - 1u), s.picture_stride, &a) || __builtin_mul_overflow((uint64_t)(h - 1u), s.pitch, &b) ||
        __builtin_add_overflow(a, b, &a) || __builtin_add_overflow(a, (uint64_t)w, &a))
        return false;
    *end = a;
    return true;
}

// The arguments of a change map, decided on the host in the order include/h263mi.h lists; *out, *sel: the launches they come to.
// cur_span: the bytes behind cur->d_base that prev may not touch under roll (0: the n pictures of cur).
static int change_args(const h263mi_plane_set *cur, const h263mi_plane_set *prev, uint32_t n, uint32_t w, uint32_t h, const h263mi_change *c,
                       uint32_t *d_cells, uint64_t cells_bytes, h263mi_change_summary *d_summary, uint32_t *d_selected, uint32_t *d_count,
                       uint64_t cur_span, ChangeArgs *out, ChangeSelectArgs *sel)
{
    uint32_t gw = 0, gh = 0;
    uint64_t extent = 0;
    RC_TRY(h263mi_change_extent(n, w, h, c, &gw, &gh, &extent));
    ChangeArgs a{};
    if (n) {
        if (!cur || !prev || !d_summary || !cur->d_base || !prev->d_base) return H263MI_ERR_INVALID_ARGUMENT;
        if (h > 1 && (cur->pitch < w || prev->pitch < w)) return H263MI_ERR_INVALID_ARGUMENT;
        uint64_t cur_end, prev_end;
        if (!plane_set_end(*cur, n, w, h, &cur_end) || cur_end > cur->bytes) return H263MI_ERR_INVALID_ARGUMENT;
        if (!plane_set_end(*prev, n, w, h, &prev_end) || prev_end > prev->bytes) return H263MI_ERR_INVALID_ARGUMENT;
        if (d_cells && cells_bytes < extent) return H263MI_ERR_INVALID_ARGUMENT;
        if (!d_selected != !d_count) return H263MI_ERR_INVALID_ARGUMENT;
        if (c->roll) {
            uint64_t one = 0;
            plane_set_end(*prev, 1, w, h, &one);                              // (no more than prev_end)
            if (n > 1 && prev->picture_stride < one) return H263MI_ERR_INVALID_ARGUMENT;
            const uintptr_t c0 = (uintptr_t)cur->d_base, p0 = (uintptr_t)prev->d_base;
            const uint64_t span = cur_span ? cur_span : cur_end;
            if (p0 < c0 + span && c0 < p0 + prev_end) return H263MI_ERR_INVALID_ARGUMENT;
        }
        a.cur = cur->d_base;
        a.prev = prev->d_base;
        a.cur_pitch = cur->pitch, a.cur_stride = cur->picture_stride;
        a.prev_pitch = prev->pitch, a.prev_stride = prev->picture_stride;
        a.cur_align = change_align(cur->d_base, cur->pitch, cur->picture_stride);
        a.prev_align = change_align(prev->d_base, prev->pitch, prev->picture_stride);
    } else if (!d_selected != !d_count) {
        return H263MI_ERR_INVALID_ARGUMENT;
    }
    a.cells = d_cells;
    a.summary = d_summary;
    a.w = w, a.h = h, a.gw = gw, a.gh = gh;
    a.cell_log2 = c->cell_log2, a.roll = c->roll, a.threshold = c->cell_threshold;
    a.n_pictures = n;
    a.segs = (w + CHANGE_SEG - 1u) / CHANGE_SEG;
    *out = a;
    *sel = ChangeSelectArgs{d_summary, nullptr, d_selected, d_count, n, c->min_changed_cells};
    return H263MI_OK;
}

// the clearing of the summaries, k_change, and k_change_select when a list is wanted, queued on `stream` of the current device
static int change_launch(const ChangeArgs &a, const ChangeSelectArgs &sel, hipStream_t stream)
{
    if (!a.n_pictures && !sel.count) return H263MI_OK;
    if (!launch_change) return H263MI_ERR_HIP;             // (kernels.h: only a stub runtime lacks it)
    auto queue = [&]() -> int {
        if (a.n_pictures) HIP_TRY(hipMemsetAsync(a.summary, 0, (size_t)a.n_pictures * sizeof(h263mi_change_summary), stream));
        HIP_TRY(launch_change(a, sel.count ? &sel : nullptr, stream));
        return H263MI_OK;
    };
    return digest_rc(queue());                             // (whatever the runtime refuses is H263MI_ERR_HIP)
}

int h263mi_batch::change_last(const h263mi_plane_set *prev, const h263mi_change *c, uint32_t *d_cells, uint64_t cells_bytes,
                              h263mi_change_summary *d_summary, uint32_t *d_selected, uint32_t *d_count, int *stream_rc)
{
    // the luma planes of the frame store, as copy_yuv reads them: set 0 at frames[0], set 1 behind it
    const uint64_t set_bytes = (uint64_t)(frames[1] - frames[0]);
    const h263mi_plane_set store{frames[0], 2 * set_bytes, L.pitch_y, L.frame_bytes};
    ChangeArgs a;
    ChangeSelectArgs sel;
    RC_TRY(change_args(&store, prev, n, L.width, L.height, c, d_cells, cells_bytes, d_summary, d_selected, d_count, store.bytes, &a, &sel));
    RC_TRY(time_close());                        // a change map is not part of any kernel's time
    std::vector<uint32_t> words(n);
    bool missing = false, same = true;
    for (uint32_t i = 0; i < n; i++) {
        words[i] = ss[i].cur < 0 ? 0u : (CHANGE_VALID | (ss[i].cur == 1 ? CHANGE_SET1 : 0u));
        missing |= ss[i].cur < 0;
        same &= words[i] == words[0];
    }
    a.cur_set1 = set_bytes;
    a.cur_align = change_align(store.d_base, store.pitch, store.picture_stride, set_bytes);
    if (same && !missing) {
        a.cur = frames[ss[0].cur];               // every stream's picture lies in one set: no words
    } else {
        const uint32_t *d_words = nullptr;
        RC_TRY(digest_rc(upload(word_ring, words.data(), &d_words, stream)));
        a.words = sel.words = d_words;
    }
    RC_TRY(change_launch(a, sel, stream));
    if (stream_rc)
        for (uint32_t i = 0; i < n; i++) stream_rc[i] = ss[i].cur < 0 ? H263MI_ERR_NO_PICTURE : H263MI_OK;
    return missing && !stream_rc ? H263MI_ERR_NO_PICTURE : H263MI_OK;
}

int h263mi_change_map_on(const h263mi_backend_cfg *cfg, const h263mi_plane_set *cur, const h263mi_plane_set *prev, uint32_t n_pictures,
                         uint32_t width, uint32_t height, const h263mi_change *c, uint32_t *d_cells, uint64_t cells_bytes,
                         h263mi_change_summary *d_summary, uint32_t *d_selected, uint32_t *d_count)
{
    ChangeArgs a;
    ChangeSelectArgs sel;
    RC_TRY(change_args(cur, prev, n_pictures, width, height, c, d_cells, cells_bytes, d_summary, d_selected, d_count, 0, &a, &sel));
    if (!n_pictures && !d_count) return H263MI_OK;
    const int dev = cfg ? cfg->device_id : 0;
    RC_TRY(check_device(dev));
    DeviceGuard g(dev);
    if (!g.ok) return H263MI_ERR_NO_DEVICE;
    return change_launch(a, sel, cfg ? (hipStream_t)cfg->stream : nullptr);
}

int h263mi_batch_change_map(h263mi_batch *b, const h263mi_plane_set *cur, const h263mi_plane_set *prev, const h263mi_change *c,
                            uint32_t *d_cells, uint64_t cells_bytes, h263mi_change_summary *d_summary, uint32_t *d_selected, uint32_t *d_count)
{
    if (!b) return H263MI_ERR_INVALID_ARGUMENT;
    ChangeArgs a;
    ChangeSelectArgs sel;
    RC_TRY(change_args(cur, prev, b->n, b->L.width, b->L.height, c, d_cells, cells_bytes, d_summary, d_selected, d_count, 0, &a, &sel));
    DeviceGuard g(b->device);
    RC_TRY(b->sync());                           // (the deferred rendering of a pipelined batch, the second stream of an overlapped one)
    return change_launch(a, sel, b->stream);
}

int h263mi_batch_change_last(h263mi_batch *b, const h263mi_plane_set *prev, const h263mi_change *c, uint32_t *d_cells, uint64_t cells_bytes,
                             h263mi_change_summary *d_summary, uint32_t *d_selected, uint32_t *d_count, int *stream_rc)
{
    if (!b) return H263MI_ERR_INVALID_ARGUMENT;
    DeviceGuard g(b->device);
    return b->change_last(prev, c, d_cells, cells_bytes, d_summary, d_selected, d_count, stream_rc);
}

// =========================================================================================
// background model (background_kernel.inl)
// =========================================================================================
int h263mi_background_extent(uint32_t n_pictures, uint32_t width, uint32_t height, const h263mi_background *bg, uint32_t *gw, uint32_t *gh,
                             uint64_t *cells_bytes, uint64_t *state_bytes)
{
    static_assert(sizeof(h263mi_background) == 16 && sizeof(h263mi_background_head) == 64, "the structures are part of the ABI");
    if (!bg || bg->reserved || bg->cell_log2 < 3 || bg->cell_log2 > 6 || bg->learn_shift > 7 ||
        (bg->fg_learn_shift > 7 && bg->fg_learn_shift != BG_KEEP))
        return H263MI_ERR_INVALID_ARGUMENT;
    if (!width || !height || width > 65535 || height > 65535 || (uint64_t)width * height >= (1ull << 30)) return H263MI_ERR_INVALID_ARGUMENT;
    if (n_pictures > CHANGE_MAX_PICTURES) return H263MI_ERR_INVALID_ARGUMENT;
    const uint32_t w = ((width - 1u) >> bg->cell_log2) + 1u, h = ((height - 1u) >> bg->cell_log2) + 1u;
    if (gw) *gw = w;
    if (gh) *gh = h;
    if (cells_bytes) *cells_bytes = (uint64_t)n_pictures * w * h * 4u;        // (below 2^16 * 2^24 * 4)
    if (state_bytes) *state_bytes = (uint64_t)n_pictures * bg_stride(width, height);     // (below 2^16 * 2^32)
    return H263MI_OK;
}

// The arguments of a background call, decided on the host in the order include/h263mi.h lists; *out, *sel: the launches they come
// to.  cur_span: the bytes behind cur->d_base that no output may touch (0: the n pictures of cur).
static int background_args(const h263mi_plane_set *cur, uint32_t n, uint32_t w, uint32_t h, const h263mi_background *bg, void *d_state,
                           uint64_t state_bytes, const uint32_t *d_cut, const uint32_t *d_cut_count, const h263mi_plane_set *mask,
                           uint32_t *d_cells, uint64_t cells_bytes, h263mi_change_summary *d_summary, uint32_t *d_selected, uint32_t *d_count,
                           uint64_t cur_span, BgArgs *out, ChangeSelectArgs *sel)
{
    uint32_t gw = 0, gh = 0;
    uint64_t cells_extent = 0, state_extent = 0;
    RC_TRY(h263mi_background_extent(n, w, h, bg, &gw, &gh, &cells_extent, &state_extent));
    BgArgs a{};
    if (n) {
        if (!cur || !d_state || !d_summary || !cur->d_base || (mask && !mask->d_base)) return H263MI_ERR_INVALID_ARGUMENT;
        if (h > 1 && (cur->pitch < w || (mask && mask->pitch < w))) return H263MI_ERR_INVALID_ARGUMENT;
        uint64_t cur_end, mask_end = 0;
        if (!plane_set_end(*cur, n, w, h, &cur_end) || cur_end > cur->bytes) return H263MI_ERR_INVALID_ARGUMENT;
        if (mask && (!plane_set_end(*mask, n, w, h, &mask_end) || mask_end > mask->bytes)) return H263MI_ERR_INVALID_ARGUMENT;
        if (state_bytes < state_extent || (d_cells && cells_bytes < cells_extent)) return H263MI_ERR_INVALID_ARGUMENT;
        if ((uintptr_t)d_state % 32) return H263MI_ERR_INVALID_ARGUMENT;
        if (!d_cut != !d_cut_count || !d_selected != !d_count) return H263MI_ERR_INVALID_ARGUMENT;
        if (mask) {
            uint64_t one = 0;
            plane_set_end(*mask, 1, w, h, &one);                             // (no more than mask_end)
            if (n > 1 && mask->picture_stride < one) return H263MI_ERR_INVALID_ARGUMENT;
        }
        // the byte ranges: the six outputs first, then the three inputs; an absent or empty one intersects nothing
        const struct {
            uintptr_t at;
            uint64_t bytes;
        } range[9] = {{(uintptr_t)d_state, state_extent},
                      {(uintptr_t)(mask ? mask->d_base : nullptr), mask_end},
                      {(uintptr_t)d_cells, d_cells ? cells_extent : 0u},
                      {(uintptr_t)d_summary, (uint64_t)n * sizeof(h263mi_change_summary)},
                      {(uintptr_t)d_selected, d_selected ? (uint64_t)n * 4u : 0u},
                      {(uintptr_t)d_count, d_count ? 4u : 0u},
                      {(uintptr_t)cur->d_base, cur_span ? cur_span : cur_end},
                      {(uintptr_t)d_cut, d_cut ? (uint64_t)n * 4u : 0u},
                      {(uintptr_t)d_cut_count, d_cut_count ? 4u : 0u}};
        for (int i = 0; i < 6; i++)
            for (int j = i + 1; j < 9; j++)
                if (range[i].bytes && range[j].bytes && range[i].at < range[j].at + range[j].bytes && range[j].at < range[i].at + range[i].bytes)
                    return H263MI_ERR_INVALID_ARGUMENT;
        a.cur = cur->d_base;
        a.cur_pitch = cur->pitch, a.cur_stride = cur->picture_stride;
        a.cur_align = change_align(cur->d_base, cur->pitch, cur->picture_stride);
        if (mask) {
            a.mask = mask->d_base;
            a.mask_pitch = mask->pitch, a.mask_stride = mask->picture_stride;
            a.mask_align = change_align(mask->d_base, mask->pitch, mask->picture_stride);
        }
    } else if (!d_cut != !d_cut_count || !d_selected != !d_count) {
        return H263MI_ERR_INVALID_ARGUMENT;
    }
    a.state = static_cast<uint8_t *>(d_state);
    a.state_stride = bg_stride(w, h);
    a.bpitch = bg_pitch(w);
    a.cut = d_cut, a.cut_count = d_cut_count;
    a.cells = d_cells;
    a.summary = d_summary;
    a.w = w, a.h = h, a.gw = gw, a.gh = gh;
    a.cell_log2 = bg->cell_log2, a.threshold = bg->cell_threshold;
    a.learn_shift = bg->learn_shift, a.fg_learn_shift = bg->fg_learn_shift, a.pixel_threshold = bg->pixel_threshold, a.warmup = bg->warmup;
    a.n_pictures = n;
    a.segs = (w + CHANGE_SEG - 1u) / CHANGE_SEG;
    *out = a;
    *sel = ChangeSelectArgs{d_summary, nullptr, d_selected, d_count, n, bg->min_changed_cells};
    return H263MI_OK;
}

// k_bg_begin, k_bg, and k_change_select when a list is wanted, queued on `stream` of the current device
static int background_launch(const BgArgs &a, const ChangeSelectArgs &sel, hipStream_t stream)
{
    if (!a.n_pictures && !sel.count) return H263MI_OK;
    if (!launch_background) return H263MI_ERR_HIP;        // (kernels.h: only a stub runtime lacks it)
    auto queue = [&]() -> int {
        HIP_TRY(launch_background(a, sel.count ? &sel : nullptr, stream));
        return H263MI_OK;
    };
    return digest_rc(queue());                             // (whatever the runtime refuses is H263MI_ERR_HIP)
}

int h263mi_batch::background_last(const h263mi_background *bg, void *d_state, uint64_t state_bytes, const uint32_t *d_cut,
                                  const uint32_t *d_cut_count, const h263mi_plane_set *mask, uint32_t *d_cells, uint64_t cells_bytes,
                                  h263mi_change_summary *d_summary, uint32_t *d_selected, uint32_t *d_count, int *stream_rc)
{
    // the luma planes of the frame store, as change_last reads them: set 0 at frames[0], set 1 behind it
    const uint64_t set_bytes = (uint64_t)(frames[1] - frames[0]);
    const h263mi_plane_set store{frames[0], 2 * set_bytes, L.pitch_y, L.frame_bytes};
    BgArgs a;
    ChangeSelectArgs sel;
    RC_TRY(background_args(&store, n, L.width, L.height, bg, d_state, state_bytes, d_cut, d_cut_count, mask, d_cells, cells_bytes, d_summary,
                           d_selected, d_count, store.bytes, &a, &sel));
    RC_TRY(time_close());                        // a background call is not part of any kernel's time
    std::vector<uint32_t> words(n);
    bool missing = false, same = true;
    for (uint32_t i = 0; i < n; i++) {
        words[i] = ss[i].cur < 0 ? 0u : (CHANGE_VALID | (ss[i].cur == 1 ? CHANGE_SET1 : 0u));
        missing |= ss[i].cur < 0;
        same &= words[i] == words[0];
    }
    a.cur_set1 = set_bytes;
    a.cur_align = change_align(store.d_base, store.pitch, store.picture_stride, set_bytes);
    if (same && !missing) {
        a.cur = frames[ss[0].cur];               // every stream's picture lies in one set: no words
    } else {
        const uint32_t *d_words = nullptr;
        RC_TRY(digest_rc(upload(word_ring, words.data(), &d_words, stream)));
        a.words = sel.words = d_words;
    }
    RC_TRY(background_launch(a, sel, stream));
    if (stream_rc)
        for (uint32_t i = 0; i < n; i++) stream_rc[i] = ss[i].cur < 0 ? H263MI_ERR_NO_PICTURE : H263MI_OK;
    return missing && !stream_rc ? H263MI_ERR_NO_PICTURE : H263MI_OK;
}

int h263mi_background_on(const h263mi_backend_cfg *cfg, const h263mi_plane_set *cur, uint32_t n_pictures, uint32_t width, uint32_t height,
                         const h263mi_background *bg, void *d_state, uint64_t state_bytes, const uint32_t *d_cut, const uint32_t *d_cut_count,
                         const h263mi_plane_set *mask, uint32_t *d_cells, uint64_t cells_bytes, h263mi_change_summary *d_summary,
                         uint32_t *d_selected, uint32_t *d_count)
{
    BgArgs a;
    ChangeSelectArgs sel;
    RC_TRY(background_args(cur, n_pictures, width, height, bg, d_state, state_bytes, d_cut, d_cut_count, mask, d_cells, cells_bytes, d_summary,
                           d_selected, d_count, 0, &a, &sel));
    if (!n_pictures && !d_count) return H263MI_OK;
    const int dev = cfg ? cfg->device_id : 0;
    RC_TRY(check_device(dev));
    DeviceGuard g(dev);
    if (!g.ok) return H263MI_ERR_NO_DEVICE;
    return background_launch(a, sel, cfg ? (hipStream_t)cfg->stream : nullptr);
}

int h263mi_batch_background(h263mi_batch *b, const h263mi_plane_set *cur, const h263mi_background *bg, void *d_state, uint64_t state_bytes,
                            const uint32_t *d_cut, const uint32_t *d_cut_count, const h263mi_plane_set *mask, uint32_t *d_cells,
                            uint64_t cells_bytes, h263mi_change_summary *d_summary, uint32_t *d_selected, uint32_t *d_count)
{
    if (!b) return H263MI_ERR_INVALID_ARGUMENT;
    BgArgs a;
    ChangeSelectArgs sel;
    RC_TRY(background_args(cur, b->n, b->L.width, b->L.height, bg, d_state, state_bytes, d_cut, d_cut_count, mask, d_cells, cells_bytes,
                           d_summary, d_selected, d_count, 0, &a, &sel));
    DeviceGuard g(b->device);
    RC_TRY(b->sync());                           // (the deferred rendering of a pipelined batch, the second stream of an overlapped one)
    return background_launch(a, sel, b->stream);
}

int h263mi_batch_background_last(h263mi_batch *b, const h263mi_background *bg, void *d_state, uint64_t state_bytes, const uint32_t *d_cut,
                                 const uint32_t *d_cut_count, const h263mi_plane_set *mask, uint32_t *d_cells, uint64_t cells_bytes,
                                 h263mi_change_summary *d_summary, uint32_t *d_selected, uint32_t *d_count, int *stream_rc)
{
    if (!b) return H263MI_ERR_INVALID_ARGUMENT;
    DeviceGuard g(b->device);
    return b->background_last(bg, d_state, state_bytes, d_cut, d_cut_count, mask, d_cells, cells_bytes, d_summary, d_selected, d_count,
                              stream_rc);
}

// =========================================================================================
// plane histograms (hist_kernel.inl)
// =========================================================================================
int h263mi_hist_extent(uint32_t n_pictures, uint32_t width, uint32_t height, const h263mi_hist *h, uint64_t *hist_bytes)
{
    static_assert(sizeof(h263mi_hist) == 16 && sizeof(h263mi_hist_stats) == 32, "the structures are part of the ABI");
    if (!h || h->reserved[0] || h->reserved[1] || h->reserved[2] || h->reserved2 || h->roll > 1) return H263MI_ERR_INVALID_ARGUMENT;
    if (h->lo_permille > 1000 || h->hi_permille > 1000 || h->cut_permille > 1000 || h->lo_permille > h->hi_permille)
        return H263MI_ERR_INVALID_ARGUMENT;
    if (!width || !height || width > 65535 || height > 65535 || (uint64_t)width * height >= (1ull << 30)) return H263MI_ERR_INVALID_ARGUMENT;
    if (n_pictures > HIST_MAX_PICTURES) return H263MI_ERR_INVALID_ARGUMENT;
    if (hist_bytes) *hist_bytes = (uint64_t)n_pictures * 1024u;
    return H263MI_OK;
}

// The arguments of a histogram call, decided on the host in the order include/h263mi.h lists; *out, *fin, *sel: the launches they
// come to.
static int hist_args(const h263mi_plane_set *set, uint32_t n, uint32_t w, uint32_t h, const h263mi_hist *d, uint32_t *d_hist, uint64_t hist_bytes,
                     uint32_t *d_prev, uint64_t prev_bytes, h263mi_hist_stats *d_stats, uint32_t *d_selected, uint32_t *d_count, HistArgs *out,
                     HistFinalArgs *fin, HistSelectArgs *sel)
{
    uint64_t extent = 0;
    RC_TRY(h263mi_hist_extent(n, w, h, d, &extent));
    HistArgs a{};
    if (n) {
        if (!set || !d_hist || !d_stats || !set->d_base) return H263MI_ERR_INVALID_ARGUMENT;
        if (h > 1 && set->pitch < w) return H263MI_ERR_INVALID_ARGUMENT;
        uint64_t end;
        if (!plane_set_end(*set, n, w, h, &end) || end > set->bytes) return H263MI_ERR_INVALID_ARGUMENT;
        if (hist_bytes < extent || (d_prev && prev_bytes < extent)) return H263MI_ERR_INVALID_ARGUMENT;
        if ((uintptr_t)d_hist % 4 || (uintptr_t)d_prev % 4 || (uintptr_t)d_stats % 8) return H263MI_ERR_INVALID_ARGUMENT;
        const uintptr_t h0 = (uintptr_t)d_hist, p0 = (uintptr_t)d_prev;
        if (d_prev && p0 < h0 + extent && h0 < p0 + extent) return H263MI_ERR_INVALID_ARGUMENT;
        a.src = set->d_base;
        a.pitch = set->pitch, a.stride = set->picture_stride;
        a.align = change_align(set->d_base, set->pitch, set->picture_stride);
    }
    if ((d->roll || d_selected || d_count) && !d_prev) return H263MI_ERR_INVALID_ARGUMENT;
    if (!d_selected != !d_count) return H263MI_ERR_INVALID_ARGUMENT;
    a.hist = d_hist;
    a.w = w, a.h = h, a.n_pictures = n;
    a.segs = (w + HIST_SEG - 1u) / HIST_SEG;
    a.bands = (h + HIST_ROWS - 1u) / HIST_ROWS;
    *out = a;
    *fin = HistFinalArgs{d_hist, d_prev, d_stats, nullptr, (uint64_t)w * h, n, d->lo_permille, d->hi_permille, d->roll};
    *sel = HistSelectArgs{d_stats, nullptr, d_selected, d_count, (uint64_t)w * h, n, d->cut_permille};
    return H263MI_OK;
}

// the clearing of the histograms, k_hist, k_hist_final, and k_hist_select when a list is wanted, queued on `stream` of the current device
static int hist_launch(const HistArgs &a, const HistFinalArgs &fin, const HistSelectArgs &sel, hipStream_t stream)
{
    if (!a.n_pictures && !sel.count) return H263MI_OK;
    if (!launch_hist) return H263MI_ERR_HIP;               // (kernels.h: only a stub runtime lacks it)
    auto queue = [&]() -> int {
        if (a.n_pictures) HIP_TRY(hipMemsetAsync(a.hist, 0, (size_t)a.n_pictures * 1024u, stream));
        HIP_TRY(launch_hist(a, fin, sel.count ? &sel : nullptr, stream));
        return H263MI_OK;
    };
    return digest_rc(queue());                             // (whatever the runtime refuses is H263MI_ERR_HIP)
}

int h263mi_batch::hist_last(uint32_t plane, const h263mi_hist *h, uint32_t *d_hist, uint64_t hist_bytes, uint32_t *d_prev_hist,
                            uint64_t prev_bytes, h263mi_hist_stats *d_stats, uint32_t *d_selected, uint32_t *d_count, int *stream_rc)
{
    if (plane > 2) return H263MI_ERR_INVALID_ARGUMENT;
    // the planes of the frame store, as copy_yuv reads them: set 0 at frames[0], set 1 behind it
    const uint64_t set_bytes = (uint64_t)(frames[1] - frames[0]), off = plane == 0 ? 0u : (plane == 1 ? L.off_cb : L.off_cr);
    const uint32_t pw = plane ? L.cwidth : L.width, ph = plane ? L.cheight : L.height;
    const h263mi_plane_set store{frames[0] + off, 2 * set_bytes - off, plane ? L.pitch_c : L.pitch_y, L.frame_bytes};
    HistArgs a;
    HistFinalArgs fin;
    HistSelectArgs sel;
    RC_TRY(hist_args(&store, n, pw, ph, h, d_hist, hist_bytes, d_prev_hist, prev_bytes, d_stats, d_selected, d_count, &a, &fin, &sel));
    RC_TRY(time_close());                        // a histogram is not part of any kernel's time
    std::vector<uint32_t> words(n);
    bool missing = false, same = true;
    for (uint32_t i = 0; i < n; i++) {
        words[i] = ss[i].cur < 0 ? 0u : (HIST_VALID | (ss[i].cur == 1 ? HIST_SET1 : 0u));
        missing |= ss[i].cur < 0;
        same &= words[i] == words[0];
    }
    a.set1 = set_bytes;
    a.align = change_align(store.d_base, store.pitch, store.picture_stride, set_bytes);
    if (same && !missing) {
        a.src = frames[ss[0].cur] + off;         // every stream's picture lies in one set: no words
    } else {
        const uint32_t *d_words = nullptr;
        RC_TRY(digest_rc(upload(word_ring, words.data(), &d_words, stream)));
        a.words = fin.words = sel.words = d_words;
    }
    RC_TRY(hist_launch(a, fin, sel, stream));
    if (stream_rc)
        for (uint32_t i = 0; i < n; i++) stream_rc[i] = ss[i].cur < 0 ? H263MI_ERR_NO_PICTURE : H263MI_OK;
    return missing && !stream_rc ? H263MI_ERR_NO_PICTURE : H263MI_OK;
}

int h263mi_hist_on(const h263mi_backend_cfg *cfg, const h263mi_plane_set *set, uint32_t n_pictures, uint32_t width, uint32_t height,
                   const h263mi_hist *h, uint32_t *d_hist, uint64_t hist_bytes, uint32_t *d_prev_hist, uint64_t prev_bytes,
                   h263mi_hist_stats *d_stats, uint32_t *d_selected, uint32_t *d_count)
{
    HistArgs a;
    HistFinalArgs fin;
    HistSelectArgs sel;
    RC_TRY(hist_args(set, n_pictures, width, height, h, d_hist, hist_bytes, d_prev_hist, prev_bytes, d_stats, d_selected, d_count, &a, &fin, &sel));
    if (!n_pictures && !d_count) return H263MI_OK;
    const int dev = cfg ? cfg->device_id : 0;
    RC_TRY(check_device(dev));
    DeviceGuard g(dev);
    if (!g.ok) return H263MI_ERR_NO_DEVICE;
    return hist_launch(a, fin, sel, cfg ? (hipStream_t)cfg->stream : nullptr);
}

int h263mi_batch_hist(h263mi_batch *b, const h263mi_plane_set *set, const h263mi_hist *h, uint32_t *d_hist, uint64_t hist_bytes,
                      uint32_t *d_prev_hist, uint64_t prev_bytes, h263mi_hist_stats *d_stats, uint32_t *d_selected, uint32_t *d_count)
{
    if (!b) return H263MI_ERR_INVALID_ARGUMENT;
    HistArgs a;
    HistFinalArgs fin;
    HistSelectArgs sel;
    RC_TRY(hist_args(set, b->n, b->L.width, b->L.height, h, d_hist, hist_bytes, d_prev_hist, prev_bytes, d_stats, d_selected, d_count, &a, &fin, &sel));
    DeviceGuard g(b->device);
    RC_TRY(b->sync());                           // (the deferred rendering of a pipelined batch, the second stream of an overlapped one)
    return hist_launch(a, fin, sel, b->stream);
}

int h263mi_batch_hist_last(h263mi_batch *b, uint32_t plane, const h263mi_hist *h, uint32_t *d_hist, uint64_t hist_bytes, uint32_t *d_prev_hist,
                           uint64_t prev_bytes, h263mi_hist_stats *d_stats, uint32_t *d_selected, uint32_t *d_count, int *stream_rc)
{
    if (!b) return H263MI_ERR_INVALID_ARGUMENT;
    DeviceGuard g(b->device);
    return b->hist_last(plane, h, d_hist, hist_bytes, d_prev_hist, prev_bytes, d_stats, d_selected, d_count, stream_rc);
}

// =========================================================================================
// motion regions (regions_kernel.inl)
// =========================================================================================
int h263mi_regions_extent(uint32_t n_pictures, uint32_t width, uint32_t height, const h263mi_regions *r, uint32_t *gw, uint32_t *gh,
                          uint64_t *cells_bytes, uint64_t *work_bytes)
{
    static_assert(sizeof(h263mi_regions) == 16 && sizeof(h263mi_region_info) == 16 && sizeof(h263mi_region_stat) == 16,
                  "the structures are part of the ABI");
    if (!r || r->reserved || r->cell_log2 < 3 || r->cell_log2 > 6 || (r->connectivity != 4 && r->connectivity != 8) ||
        r->margin_cells > REGIONS_MAX_MARGIN || !r->min_cells || !r->max_per_picture || r->max_per_picture > REGIONS_MAX_PER_PICTURE)
        return H263MI_ERR_INVALID_ARGUMENT;
    if (!width || !height || width > 65535 || height > 65535 || (uint64_t)width * height >= (1ull << 30)) return H263MI_ERR_INVALID_ARGUMENT;
    if (n_pictures > CHANGE_MAX_PICTURES) return H263MI_ERR_INVALID_ARGUMENT;
    const uint32_t w = ((width - 1u) >> r->cell_log2) + 1u, h = ((height - 1u) >> r->cell_log2) + 1u;
    if ((uint64_t)w * h > REGIONS_MAX_CELLS) return H263MI_ERR_INVALID_ARGUMENT;
    if (gw) *gw = w;
    if (gh) *gh = h;
    if (cells_bytes) *cells_bytes = (uint64_t)n_pictures * w * h * 4u;
    if (work_bytes) *work_bytes = (uint64_t)n_pictures * r->max_per_picture * REGIONS_ENTRY;
    return H263MI_OK;
}

// The arguments of a regions call, decided on the host in the order include/h263mi.h lists; *out, *pack: the launches they come to.
static int regions_args(const uint32_t *d_cells, uint64_t cells_bytes, const h263mi_change_summary *d_summary, uint32_t n, uint32_t w,
                        uint32_t h, const h263mi_regions *r, void *d_work, uint64_t work_bytes, h263mi_roi *d_rois, uint32_t max_rois,
                        h263mi_region_stat *d_stats, h263mi_region_info *d_info, uint32_t *d_count, RegionsArgs *out, RegionsPackArgs *pack)
{
    uint32_t gw = 0, gh = 0;
    uint64_t cells_extent = 0, work_extent = 0;
    RC_TRY(h263mi_regions_extent(n, w, h, r, &gw, &gh, &cells_extent, &work_extent));
    if (!d_rois || !d_count) return H263MI_ERR_INVALID_ARGUMENT;
    if (n && (!d_cells || !d_work || !d_info)) return H263MI_ERR_INVALID_ARGUMENT;
    if (cells_bytes < cells_extent || work_bytes < work_extent) return H263MI_ERR_INVALID_ARGUMENT;
    if (!max_rois || max_rois > REGIONS_MAX_ROIS) return H263MI_ERR_INVALID_ARGUMENT;
    if ((uintptr_t)d_cells % 4 || (uintptr_t)d_rois % 4 || (uintptr_t)d_info % 4 || (uintptr_t)d_count % 4 || (uintptr_t)d_work % 8 ||
        (uintptr_t)d_stats % 8 || (uintptr_t)d_summary % 8)
        return H263MI_ERR_INVALID_ARGUMENT;
    // the byte ranges: the five outputs first, then the two inputs; an absent or empty one intersects nothing
    const struct {
        uintptr_t at;
        uint64_t bytes;
    } range[7] = {{(uintptr_t)d_rois, (uint64_t)max_rois * sizeof(h263mi_roi)},
                  {(uintptr_t)d_stats, d_stats ? (uint64_t)max_rois * sizeof(h263mi_region_stat) : 0u},
                  {(uintptr_t)d_info, (uint64_t)n * sizeof(h263mi_region_info)},
                  {(uintptr_t)d_count, 8u},
                  {(uintptr_t)d_work, work_extent},
                  {(uintptr_t)d_cells, cells_extent},
                  {(uintptr_t)d_summary, d_summary ? (uint64_t)n * sizeof(h263mi_change_summary) : 0u}};
    for (int i = 0; i < 5; i++)
        for (int j = i + 1; j < 7; j++)
            if (range[i].bytes && range[j].bytes && range[i].at < range[j].at + range[j].bytes && range[j].at < range[i].at + range[i].bytes)
                return H263MI_ERR_INVALID_ARGUMENT;
    RegionsArgs a{};
    a.cells = d_cells;
    a.summary = d_summary;
    a.work = static_cast<uint8_t *>(d_work);
    a.info = d_info;
    a.w = w, a.h = h, a.gw = gw, a.gh = gh;
    a.cell_log2 = r->cell_log2, a.connectivity = r->connectivity, a.margin = r->margin_cells, a.threshold = r->cell_threshold;
    a.min_cells = r->min_cells, a.max_per = r->max_per_picture, a.n_pictures = n;
    *out = a;
    *pack = RegionsPackArgs{d_summary, a.work, d_rois, d_stats, d_info, d_count, n, r->max_per_picture, max_rois, 0};
    return H263MI_OK;
}

// k_regions over the pictures and k_regions_pack, queued on `stream` of the current device
static int regions_launch(const RegionsArgs &a, const RegionsPackArgs &pack, hipStream_t stream)
{
    if (!launch_regions) return H263MI_ERR_HIP;            // (kernels.h: only a stub runtime lacks it)
    auto queue = [&]() -> int {
        HIP_TRY(launch_regions(a, pack, stream));
        return H263MI_OK;
    };
    return digest_rc(queue());                             // (whatever the runtime refuses is H263MI_ERR_HIP)
}

int h263mi_regions_on(const h263mi_backend_cfg *cfg, const uint32_t *d_cells, uint64_t cells_bytes, const h263mi_change_summary *d_summary,
                      uint32_t n_pictures, uint32_t width, uint32_t height, const h263mi_regions *r, void *d_work, uint64_t work_bytes,
                      h263mi_roi *d_rois, uint32_t max_rois, h263mi_region_stat *d_stats, h263mi_region_info *d_info, uint32_t *d_count)
{
    RegionsArgs a;
    RegionsPackArgs pack;
    RC_TRY(regions_args(d_cells, cells_bytes, d_summary, n_pictures, width, height, r, d_work, work_bytes, d_rois, max_rois, d_stats, d_info,
                        d_count, &a, &pack));
    const int dev = cfg ? cfg->device_id : 0;
    RC_TRY(check_device(dev));
    DeviceGuard g(dev);
    if (!g.ok) return H263MI_ERR_NO_DEVICE;
    return regions_launch(a, pack, cfg ? (hipStream_t)cfg->stream : nullptr);
}

int h263mi_batch_regions(h263mi_batch *b, const uint32_t *d_cells, uint64_t cells_bytes, const h263mi_change_summary *d_summary,
                         const h263mi_regions *r, void *d_work, uint64_t work_bytes, h263mi_roi *d_rois, uint32_t max_rois,
                         h263mi_region_stat *d_stats, h263mi_region_info *d_info, uint32_t *d_count)
{
    if (!b) return H263MI_ERR_INVALID_ARGUMENT;
    RegionsArgs a;
    RegionsPackArgs pack;
    RC_TRY(regions_args(d_cells, cells_bytes, d_summary, b->n, b->L.width, b->L.height, r, d_work, work_bytes, d_rois, max_rois, d_stats,
                        d_info, d_count, &a, &pack));
    DeviceGuard g(b->device);
    RC_TRY(b->sync());                           // (the deferred rendering of a pipelined batch, the second stream of an overlapped one)
    return regions_launch(a, pack, b->stream);
}

// =========================================================================================
// region tracks (tracks_kernel.inl)
// =========================================================================================
int h263mi_tracks_extent(uint32_t n_pictures, uint32_t width, uint32_t height, const h263mi_tracks *t, uint64_t *state_bytes)
{
    static_assert(sizeof(h263mi_tracks) == 16 && sizeof(h263mi_track) == 32 && sizeof(h263mi_track_head) == 32 &&
                      sizeof(h263mi_track_info) == 32 && sizeof(h263mi_track_ref) == 16,
                  "the structures are part of the ABI");
    if (!t || t->reserved || !t->max_tracks || t->max_tracks > TRACKS_MAX || t->iou_permille > 1000 || t->max_missed == 65535 || !t->min_hits)
        return H263MI_ERR_INVALID_ARGUMENT;
    if (!width || !height || width > 65535 || height > 65535 || (uint64_t)width * height >= (1ull << 30)) return H263MI_ERR_INVALID_ARGUMENT;
    if (n_pictures > TRACKS_MAX_PICTURES) return H263MI_ERR_INVALID_ARGUMENT;
    if (state_bytes) *state_bytes = (uint64_t)n_pictures * tracks_stride(t->max_tracks);
    return H263MI_OK;
}

// The arguments of a tracks call, decided on the host in the order include/h263mi.h lists; *out, *pack: the launches they come to.
static int tracks_args(const h263mi_roi *d_rois, uint32_t n_rois, const h263mi_region_info *d_info_in, uint32_t n, uint32_t w, uint32_t h,
                       const h263mi_tracks *t, void *d_state, uint64_t state_bytes, const uint32_t *d_cut, const uint32_t *d_cut_count,
                       h263mi_roi *d_out_rois, uint32_t max_out, h263mi_track_ref *d_out_refs, h263mi_track_info *d_info, uint32_t *d_count,
                       TracksArgs *out, TracksPackArgs *pack)
{
    uint64_t extent = 0;
    RC_TRY(h263mi_tracks_extent(n, w, h, t, &extent));
    if (!d_out_rois || !d_count) return H263MI_ERR_INVALID_ARGUMENT;
    if (n && (!d_info_in || !d_state || !d_info || (n_rois && !d_rois))) return H263MI_ERR_INVALID_ARGUMENT;
    if (n_rois > TRACKS_MAX_ROIS) return H263MI_ERR_INVALID_ARGUMENT;
    if (!max_out || max_out > TRACKS_MAX_OUT) return H263MI_ERR_INVALID_ARGUMENT;
    if (state_bytes < extent) return H263MI_ERR_INVALID_ARGUMENT;
    if (!d_cut != !d_cut_count) return H263MI_ERR_INVALID_ARGUMENT;
    if ((uintptr_t)d_rois % 4 || (uintptr_t)d_info_in % 4 || (uintptr_t)d_cut % 4 || (uintptr_t)d_cut_count % 4 || (uintptr_t)d_out_rois % 4 ||
        (uintptr_t)d_out_refs % 4 || (uintptr_t)d_info % 4 || (uintptr_t)d_count % 4 || (uintptr_t)d_state % 8)
        return H263MI_ERR_INVALID_ARGUMENT;
    // the byte ranges: the five outputs first, then the four inputs; an absent or empty one intersects nothing
    const struct {
        uintptr_t at;
        uint64_t bytes;
    } range[9] = {{(uintptr_t)d_state, extent},
                  {(uintptr_t)d_out_rois, (uint64_t)max_out * sizeof(h263mi_roi)},
                  {(uintptr_t)d_out_refs, d_out_refs ? (uint64_t)max_out * sizeof(h263mi_track_ref) : 0u},
                  {(uintptr_t)d_info, (uint64_t)n * sizeof(h263mi_track_info)},
                  {(uintptr_t)d_count, 8u},
                  {(uintptr_t)d_rois, d_rois ? (uint64_t)n_rois * sizeof(h263mi_roi) : 0u},
                  {(uintptr_t)d_info_in, (uint64_t)n * sizeof(h263mi_region_info)},
                  {(uintptr_t)d_cut, d_cut ? (uint64_t)n * 4u : 0u},
                  {(uintptr_t)d_cut_count, d_cut_count ? 4u : 0u}};
    for (int i = 0; i < 5; i++)
        for (int j = i + 1; j < 9; j++)
            if (range[i].bytes && range[j].bytes && range[i].at < range[j].at + range[j].bytes && range[j].at < range[i].at + range[i].bytes)
                return H263MI_ERR_INVALID_ARGUMENT;
    TracksArgs a{};
    a.rois = d_rois, a.info_in = d_info_in;
    a.state = static_cast<uint8_t *>(d_state);
    a.cut = d_cut, a.cut_count = d_cut_count;
    a.info = d_info;
    a.n_rois = n_rois, a.n_pictures = n, a.w = w, a.h = h;
    a.max_tracks = t->max_tracks, a.iou_permille = t->iou_permille, a.max_missed = t->max_missed, a.min_hits = t->min_hits;
    a.emit_period = t->emit_period;
    *out = a;
    *pack = TracksPackArgs{a.state, d_out_rois, d_out_refs, d_info, d_count, n, t->max_tracks, max_out, 0};
    return H263MI_OK;
}

// k_tracks over the pictures and k_tracks_pack, queued on `stream` of the current device
static int tracks_launch(const TracksArgs &a, const TracksPackArgs &pack, hipStream_t stream)
{
    if (!launch_tracks) return H263MI_ERR_HIP;             // (kernels.h: only a stub runtime lacks it)
    auto queue = [&]() -> int {
        HIP_TRY(launch_tracks(a, pack, stream));
        return H263MI_OK;
    };
    return digest_rc(queue());                             // (whatever the runtime refuses is H263MI_ERR_HIP)
}

int h263mi_tracks_on(const h263mi_backend_cfg *cfg, const h263mi_roi *d_rois, uint32_t n_rois, const h263mi_region_info *d_info_in,
                     uint32_t n_pictures, uint32_t width, uint32_t height, const h263mi_tracks *t, void *d_state, uint64_t state_bytes,
                     const uint32_t *d_cut, const uint32_t *d_cut_count, h263mi_roi *d_out_rois, uint32_t max_out,
                     h263mi_track_ref *d_out_refs, h263mi_track_info *d_info, uint32_t *d_count)
{
    TracksArgs a;
    TracksPackArgs pack;
    RC_TRY(tracks_args(d_rois, n_rois, d_info_in, n_pictures, width, height, t, d_state, state_bytes, d_cut, d_cut_count, d_out_rois, max_out,
                       d_out_refs, d_info, d_count, &a, &pack));
    const int dev = cfg ? cfg->device_id : 0;
    RC_TRY(check_device(dev));
    DeviceGuard g(dev);
    if (!g.ok) return H263MI_ERR_NO_DEVICE;
    return tracks_launch(a, pack, cfg ? (hipStream_t)cfg->stream : nullptr);
}

int h263mi_batch_tracks(h263mi_batch *b, const h263mi_roi *d_rois, uint32_t n_rois, const h263mi_region_info *d_info_in,
                        const h263mi_tracks *t, void *d_state, uint64_t state_bytes, const uint32_t *d_cut, const uint32_t *d_cut_count,
                        h263mi_roi *d_out_rois, uint32_t max_out, h263mi_track_ref *d_out_refs, h263mi_track_info *d_info, uint32_t *d_count)
{
    if (!b) return H263MI_ERR_INVALID_ARGUMENT;
    TracksArgs a;
    TracksPackArgs pack;
    RC_TRY(tracks_args(d_rois, n_rois, d_info_in, b->n, b->L.width, b->L.height, t, d_state, state_bytes, d_cut, d_cut_count, d_out_rois,
                       max_out, d_out_refs, d_info, d_count, &a, &pack));
    DeviceGuard g(b->device);
    RC_TRY(b->sync());                           // (the deferred rendering of a pipelined batch, the second stream of an overlapped one)
    return tracks_launch(a, pack, b->stream);
}

int h263mi_batch_timing_begin(h263mi_batch *b)
{
    if (!b) return H263MI_ERR_INVALID_ARGUMENT;
    b->timing = true;
    b->ev_used = 0;
    b->ev_ranges.clear();
    b->chain_kernel = -1;
    return H263MI_OK;
}

int h263mi_batch_timing_reserve(h263mi_batch *b, uint32_t n_launches)
{
    if (!b) return H263MI_ERR_INVALID_ARGUMENT;
    DeviceGuard g(b->device);
    while (b->ev_pool.size() < 2 * (size_t)n_launches) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        b->ev_pool.push_back(e);
    }
    b->ev_ranges.reserve(n_launches);
    return H263MI_OK;
}

int h263mi_batch_timing_end(h263mi_batch *b, h263mi_kernel_times *out)
{
    if (!b || !out) return H263MI_ERR_INVALID_ARGUMENT;
    DeviceGuard g(b->device);
    RC_TRY(b->time_close());
    b->timing = false;
    if (b->overlap_post) HIP_TRY(hipStreamSynchronize(b->post_stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    *out = h263mi_kernel_times{};
    for (auto &r : b->ev_ranges) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, b->ev_pool[r.first], b->ev_pool[r.first + 1]));
        if (r.kernel == 0) {
            out->recon_ms += ms;
            out->recon_launches += r.launches;
        } else if (r.kernel == 1 || r.kernel == 3) {       // (3: k_rgba_resize, the second half of a resized rendering)
            out->post_ms += ms;
            out->post_launches += r.launches;
        } else if (r.kernel == 4 || r.kernel == 5) {       // (k_plane_resize, k_plane_filter: post-processing time of the renderings counted above)
            out->post_ms += ms;
        } else {
            out->frame_ms += ms;
            out->frame_launches += r.launches;
        }
    }
    b->ev_ranges.clear();
    b->ev_used = 0;
    return H263MI_OK;
}

}  // extern "C"
