// mixed_set.cpp -- streams of DIFFERENT picture sizes behind one call (h263mi_mixed_*)
//
// The reference resolves the picture format per H263State and per picture (state.rs:157-176): a server holds QCIF, CIF
// and 1080p streams side by side, and a stream may change its size at an I picture.  A fixed-geometry batch (above)
// takes one size; h263mi_mixed keeps one such batch per size CLASS -- created when the first stream of that size
// shows up -- and a call decodes every class that has pictures in it with ONE launch (k_frame on pipelined classes), back
// to back on the same HIP stream.  A stream belongs to the class of its last picture; an I picture of another size moves
// it (its old slot is given up once the new picture's launch is queued), a picture of another size with inter
// macroblocks is that stream's H263MI_ERR_PICTURE_FORMAT_INVALID (the reference indexes the new planes with the old
// strides there, gather.rs:150,183).
//
// Round 5: SLOTS BY MEMBERSHIP.  A class owns as many slots as it has (had) members -- a power of two, doubled when a
// stream joins a full class, halved when three quarters of it stand empty -- and a map stream <-> slot; its frame store
// is 2 x slots frames and its launches cover its slots, not the streams of the whole set (round 4: every class held two
// frames for every stream of the set: 63 QCIF streams and one 1080p stream cost 64 x 2 x 3.1 MB for the one).  Growing
// and shrinking move the members' frames into a new batch (device-to-device copies behind a sync of the old one: rare).
// =========================================================================================
#include "batch.h"

#include <algorithm>
#include <cstring>
#include <new>

using namespace h263mi;

struct h263mi_mixed {
    uint32_t n = 0;
    h263mi_backend_cfg cfg{};
    struct SizeClass {
        uint32_t w = 0, h = 0;
        h263mi_batch *b = nullptr;              // b->n slots
        std::vector<int> stream_of_slot;        // -1 = free
        bool submitted = false;                 // took part in the current call
        uint32_t members() const
        {
            uint32_t k = 0;
            for (int s : stream_of_slot) k += s >= 0 ? 1u : 0u;
            return k;
        }
        // slot s is free again, its stream state forgotten (the frames are not touched: a rendering of its last picture that
        // is still pending is delivered all the same)
        void free_slot(int s)
        {
            const bool a = b->ss[s].active;
            b->ss[s] = h263mi_batch::StreamState();
            b->ss[s].active = a;
            stream_of_slot[s] = -1;
        }
    };
    std::vector<SizeClass> classes;
    struct Want { uint32_t w, h; };             // the size a stream's picture of the current call has
    std::vector<int> cls;                       // per stream: index into `classes`, -1 = no picture yet
    std::vector<int> slot;                      // per stream: its slot in that class
    std::vector<int> late_rc;                   // per stream: a device error found while its class was rebuilt, reported by the next sync
    std::vector<bits::ParserContext> parser_ctx;
    std::vector<bits::ParsedPicture> parsed;
    HostPlacement placement;                    // the NUMA node of the set's device (worker_pool.h)
    std::unique_ptr<WorkerPool> pool;
    // What the frame stores of all classes together may take (0 = no limit).  The sizes come out of untrusted bitstreams:
    // without a limit one hostile key frame of 16 384 x 16 384 asks for 800 MB per stream that sends one.
    uint64_t limit_bytes = 0;
    // h263mi_mixed_set_rgba_resize: every stream rendered as W' x H' (offsets NULL), or full size (resized false)
    bool resized = false;
    h263mi_rgba_resize resize{};
    // h263mi_mixed_set_tensor_output: every stream written as the 3 x H' x W' tensor (stride_n 0) -- in the place of a resize
    bool tensored = false;
    h263mi_tensor_out tensor{};
    uint64_t tensor_bytes = 0;                  // h263mi_tensor_extent(1, &tensor)
    // h263mi_mixed_set_*_framed: the framing of the resize or tensor in force (never WINDOW), resolved per size class
    bool framed = false;
    h263mi_framing framing{};
    // h263mi_mixed_set_*_filtered: the filter of the resize or tensor in force (AREA: none); every class has its own tap tables
    h263mi_filter filter{};
    ~h263mi_mixed()
    {
        pool.reset();                           // the host threads first
        for (SizeClass &c : classes) delete c.b;
    }
    // a class's frame store, and the scratch of its full-size pictures while a resize that is not a layout is in force, or a
    // tensor (which always has one)
    static uint64_t class_bytes(uint32_t w, uint32_t h, uint32_t slots, const h263mi_rgba_resize *rz, const h263mi_tensor_out *t = nullptr,
                                const h263mi_framing *f = nullptr, const h263mi_filter *flt = nullptr)
    {
        return 2ull * slots * make_layout(w, h).frame_bytes +
               (t ? tensor_scratch_bytes(w, h, slots, *t, f, flt) : (rz ? resize_scratch_bytes(w, h, slots, *rz, f, flt) : 0));
    }
    uint64_t slots_bytes(uint32_t w, uint32_t h, uint32_t slots) const
    {
        return class_bytes(w, h, slots, resized ? &resize : nullptr, tensored ? &tensor : nullptr, framed ? &framing : nullptr, &filter);
    }
    // the output shape in force for a class of `slots` slots of w x h (each slot placed by its own pointer)
    int class_shape(uint32_t slots, uint32_t w, uint32_t h, h263mi_batch::RgbaLayout &out) const
    {
        if (tensored) return make_tensor_shape(cfg.device_id, slots, w, h, &tensor, out, framed ? &framing : nullptr, &filter);
        return make_output_shape(cfg.device_id, slots, w, h, resized ? &resize : nullptr, out, framed ? &framing : nullptr, &filter);
    }
    uint64_t store_bytes() const
    {
        uint64_t sum = 0;
        for (const SizeClass &c : classes)
            if (c.b) sum += slots_bytes(c.w, c.h, c.b->n);
        return sum;
    }
    // what stream s's buffer must hold for a picture of w x h
    uint64_t rgba_need(uint32_t w, uint32_t h) const
    {
        if (tensored) return tensor_bytes;
        if (!resized) return (uint64_t)w * h * 4;
        const uint64_t row = 4ull * resize.out_width, pitch = resize.row_pitch ? resize.row_pitch : row;
        return (uint64_t)(resize.out_height - 1) * pitch + row;
    }
    WorkerPool &workers(unsigned want)
    {
        if (!pool || pool->size() < want) pool.reset(new WorkerPool(want - 1, &placement));
        return *pool;
    }
    static uint32_t pow2_at_least(uint32_t v)
    {
        uint32_t p = 1;
        while (p < v) p <<= 1;
        return p;
    }
    int find_class(uint32_t w, uint32_t h) const
    {
        for (size_t k = 0; k < classes.size(); k++)
            if (classes[k].b && classes[k].w == w && classes[k].h == h) return (int)k;
        return -1;
    }
    // classes nobody belongs to and nobody is about to join give up their batch: the dimensions come out of untrusted
    // bitstreams, and a stream that changes its size with every key frame must not make the set grow
    // (target[i] == -2: stream i joins a class of size want[i] that has not been resolved yet -- an existing class of that
    // size is wanted too: dropping it now would free its frame store and staging only to make them again a moment later)
    void drop_empty_classes(const std::vector<int> &target, const std::vector<Want> &want)
    {
        for (size_t k = 0; k < classes.size(); k++) {
            if (!classes[k].b || classes[k].members()) continue;
            bool wanted = false;
            for (uint32_t i = 0; i < n && !wanted; i++)
                wanted = target[i] == (int)k || (target[i] == -2 && want[i].w == classes[k].w && want[i].h == classes[k].h);
            if (wanted) continue;
            // (a rendering of a picture a departed stream left behind is delivered first; the destructor waits for it)
            if (classes[k].b->pending.valid) (void)classes[k].b->flush_pending();
            delete classes[k].b;
            classes[k] = SizeClass();
        }
    }
    // a batch of `slots` slots for class k in the place of the one it has (or of none): the members move over, slot by slot
    // from 0 on.  The old batch is synced first (a device error found there is kept in late_rc for h263mi_mixed_sync).
    int rebuild_class(size_t k, uint32_t slots)
    {
        SizeClass &c = classes[k];
        h263mi_batch *ob = c.b;
        const uint64_t others = store_bytes() - (ob ? slots_bytes(c.w, c.h, ob->n) : 0);
        // (old and new exist side by side for the length of the copies)
        if (limit_bytes && others + slots_bytes(c.w, c.h, slots) + (ob ? slots_bytes(c.w, c.h, ob->n) : 0) > limit_bytes)
            return H263MI_ERR_OUT_OF_MEMORY;
        h263mi_batch *nb = nullptr;
        RC_TRY(batch_create(slots, c.w, c.h, &cfg, &nb));
        {
            const int rc = class_shape(slots, c.w, c.h, nb->layout);
            if (rc != H263MI_OK) {
                delete nb;
                return rc;
            }
        }
        std::vector<int> moved(slots, -1);
        if (ob) {
            std::vector<int> rcs(ob->n, H263MI_OK);
            const int src = ob->sync(rcs.data());           // (delivers a deferred rendering too)
            if (src != H263MI_OK && src != H263MI_ERR_UNCODED_IFRAME_BLOCKS && src != H263MI_ERR_INVALID_ARGUMENT) {
                delete nb;
                return src;
            }
            uint32_t at = 0;
            for (uint32_t s = 0; s < ob->n; s++) {
                const int i = c.stream_of_slot[s];
                if (i < 0) continue;
                if (rcs[s] != H263MI_OK && late_rc[i] == H263MI_OK) late_rc[i] = rcs[s];
                for (int set = 0; set < 2; set++) {
                    const hipError_t e = fault_now() ? hipErrorOutOfMemory
                        : hipMemcpyAsync(nb->frames[set] + (size_t)at * nb->L.frame_bytes, ob->frames[set] + (size_t)s * ob->L.frame_bytes,
                                         ob->L.frame_bytes, hipMemcpyDeviceToDevice, ob->stream);
                    if (e != hipSuccess) {
                        (void)hipStreamSynchronize(ob->stream);
                        delete nb;
                        return map_hip_error(e);
                    }
                }
                nb->ss[at] = ob->ss[s];
                moved[at] = i;
                at++;
            }
            // the copies read the old frame store: it may go when they are done
            if (hipStreamSynchronize(ob->stream) != hipSuccess) {
                delete nb;
                return H263MI_ERR_HIP;
            }
            for (uint32_t s = 0; s < slots; s++) {
                const int i = moved[s];
                if (i < 0) continue;
                if (cls[i] == (int)k) slot[i] = (int)s;
            }
            delete ob;
        }
        c.b = nb;
        c.stream_of_slot = moved;
        return H263MI_OK;
    }
    uint32_t live_classes() const
    {
        uint32_t k = 0;
        for (const SizeClass &c : classes) k += c.b ? 1u : 0u;
        return k;
    }
};

extern "C" {

int h263mi_mixed_create(uint32_t n_streams, const h263mi_backend_cfg *cfg, h263mi_mixed **out)
{
    if (!out || !n_streams) return H263MI_ERR_INVALID_ARGUMENT;
    const int dev = cfg ? cfg->device_id : 0;
    RC_TRY(check_device(dev));
    h263mi_mixed *m = new (std::nothrow) h263mi_mixed();
    if (!m) return H263MI_ERR_OUT_OF_MEMORY;
    m->n = n_streams;
    if (cfg) m->cfg = *cfg;
    m->cfg.device_id = dev;
    m->cfg.flags &= ~H263MI_CFG_OVERLAP_POST;     // (one HIP stream carries the classes' launches back to back)
    {
        // default limit: half of the device's memory
        DeviceGuard g(dev);
        size_t free_b = 0, total_b = 0;
        if (g.ok && hipMemGetInfo(&free_b, &total_b) == hipSuccess) m->limit_bytes = total_b / 2;
        if (g.ok) m->placement = placement_of_device(dev);
    }
    m->cls.assign(n_streams, -1);
    m->slot.assign(n_streams, -1);
    m->late_rc.assign(n_streams, H263MI_OK);
    m->parser_ctx.assign(n_streams, bits::ParserContext());
    m->parsed.resize(n_streams);
    *out = m;
    return H263MI_OK;
}

void h263mi_mixed_destroy(h263mi_mixed *m) { delete m; }

int h263mi_mixed_stream_size(const h263mi_mixed *m, uint32_t stream, uint16_t *width, uint16_t *height)
{
    if (!m || stream >= m->n) return H263MI_ERR_INVALID_ARGUMENT;
    const int c = m->cls[stream];
    const bool has = c >= 0 && m->classes[c].b->ss[m->slot[stream]].cur >= 0;
    if (width) *width = has ? (uint16_t)m->classes[c].w : 0;
    if (height) *height = has ? (uint16_t)m->classes[c].h : 0;
    return has ? H263MI_OK : H263MI_ERR_NO_PICTURE;
}

uint32_t h263mi_mixed_size_classes(const h263mi_mixed *m) { return m ? m->live_classes() : 0; }

int h263mi_mixed_set_memory_limit(h263mi_mixed *m, uint64_t bytes)
{
    if (!m) return H263MI_ERR_INVALID_ARGUMENT;
    m->limit_bytes = bytes;
    return H263MI_OK;
}

uint64_t h263mi_mixed_frame_store_bytes(const h263mi_mixed *m) { return m ? m->store_bytes() : 0; }

// what a framing of a mixed set must say whatever the sizes: valid, and not a WINDOW (f may be null; 1 x 1 -> ow x oh resolves
// under the rules that do not depend on the picture)
static int mixed_framing_ok(const h263mi_framing *f, uint32_t ow, uint32_t oh)
{
    if (!f) return H263MI_OK;
    if (f->mode == H263MI_FRAME_WINDOW) return H263MI_ERR_INVALID_ARGUMENT;
    h263mi_framing_rects rc;
    return framing_resolve(1, 1, ow, oh, f, &rc);
}

int h263mi_mixed_set_rgba_resize(h263mi_mixed *m, const h263mi_rgba_resize *r) { return h263mi_mixed_set_rgba_resize_framed(m, r, nullptr); }

int h263mi_mixed_set_rgba_resize_framed(h263mi_mixed *m, const h263mi_rgba_resize *r, const h263mi_framing *f)
{
    return h263mi_mixed_set_rgba_resize_filtered(m, r, f, nullptr);
}

int h263mi_mixed_set_rgba_resize_filtered(h263mi_mixed *m, const h263mi_rgba_resize *r, const h263mi_framing *f, const h263mi_filter *flt)
{
    if (!m || (r && r->offsets)) return H263MI_ERR_INVALID_ARGUMENT;
    if (r) RC_TRY(rgba_resize_extent(1, r, nullptr));
    if (!r) f = nullptr, flt = nullptr;
    RC_TRY(filter_kind(flt));
    if (r) RC_TRY(mixed_framing_ok(f, r->out_width, r->out_height));
    DeviceGuard g(m->cfg.device_id);
    if (!g.ok) return H263MI_ERR_NO_DEVICE;
    // every class's new shape first (the scratches they need count against the limit), then all of them at once
    uint64_t total = 0;
    for (const h263mi_mixed::SizeClass &c : m->classes)
        if (c.b) total += h263mi_mixed::class_bytes(c.w, c.h, c.b->n, r, nullptr, f, flt);
    if (m->limit_bytes && total > m->limit_bytes) return H263MI_ERR_OUT_OF_MEMORY;
    std::vector<h263mi_batch::RgbaLayout> shapes(m->classes.size());
    for (size_t k = 0; k < m->classes.size(); k++)
        if (m->classes[k].b) RC_TRY(make_output_shape(m->cfg.device_id, m->classes[k].b->n, m->classes[k].w, m->classes[k].h, r, shapes[k], f, flt));
    for (size_t k = 0; k < m->classes.size(); k++)
        if (m->classes[k].b) m->classes[k].b->layout = std::move(shapes[k]);
    m->resized = r != nullptr;
    m->resize = r ? *r : h263mi_rgba_resize{};
    m->tensored = false;
    m->framed = f != nullptr;
    m->framing = f ? *f : h263mi_framing{};
    m->filter = flt ? *flt : h263mi_filter{};
    return H263MI_OK;
}

int h263mi_mixed_set_tensor_output(h263mi_mixed *m, const h263mi_tensor_out *t) { return h263mi_mixed_set_tensor_output_framed(m, t, nullptr); }

int h263mi_mixed_set_tensor_output_framed(h263mi_mixed *m, const h263mi_tensor_out *t, const h263mi_framing *f)
{
    return h263mi_mixed_set_tensor_output_filtered(m, t, f, nullptr);
}

int h263mi_mixed_set_tensor_output_filtered(h263mi_mixed *m, const h263mi_tensor_out *t, const h263mi_framing *f, const h263mi_filter *flt)
{
    if (!m || (t && t->stride_n)) return H263MI_ERR_INVALID_ARGUMENT;
    uint64_t one = 0;
    if (t) RC_TRY(tensor_extent(1, t, &one));
    if (!t) f = nullptr, flt = nullptr;
    RC_TRY(filter_kind(flt));
    if (t) RC_TRY(mixed_framing_ok(f, t->out_width, t->out_height));
    DeviceGuard g(m->cfg.device_id);
    if (!g.ok) return H263MI_ERR_NO_DEVICE;
    // every class's new shape first (the scratches they need count against the limit), then all of them at once
    uint64_t total = 0;
    for (const h263mi_mixed::SizeClass &c : m->classes)
        if (c.b) total += h263mi_mixed::class_bytes(c.w, c.h, c.b->n, nullptr, t, f, flt);
    if (m->limit_bytes && total > m->limit_bytes) return H263MI_ERR_OUT_OF_MEMORY;
    std::vector<h263mi_batch::RgbaLayout> shapes(m->classes.size());
    for (size_t k = 0; k < m->classes.size(); k++)
        if (m->classes[k].b) RC_TRY(make_tensor_shape(m->cfg.device_id, m->classes[k].b->n, m->classes[k].w, m->classes[k].h, t, shapes[k], f, flt));
    for (size_t k = 0; k < m->classes.size(); k++)
        if (m->classes[k].b) m->classes[k].b->layout = std::move(shapes[k]);
    m->tensored = t != nullptr;
    m->tensor = t ? *t : h263mi_tensor_out{};
    m->tensor_bytes = one;
    m->resized = false;
    m->resize = h263mi_rgba_resize{};
    m->framed = f != nullptr;
    m->framing = f ? *f : h263mi_framing{};
    m->filter = flt ? *flt : h263mi_filter{};
    return H263MI_OK;
}

int h263mi_mixed_stream_framing(const h263mi_mixed *m, uint32_t stream, h263mi_framing_rects *out)
{
    if (!m || stream >= m->n || !out) return H263MI_ERR_INVALID_ARGUMENT;
    const int c = m->cls[stream];
    if (c < 0 || m->classes[c].b->ss[m->slot[stream]].cur < 0) return H263MI_ERR_NO_PICTURE;
    const uint32_t w = m->classes[c].w, h = m->classes[c].h;
    const uint32_t ow = m->tensored ? m->tensor.out_width : (m->resized ? m->resize.out_width : w);
    const uint32_t oh = m->tensored ? m->tensor.out_height : (m->resized ? m->resize.out_height : h);
    return framing_resolve(w, h, ow, oh, m->framed ? &m->framing : nullptr, out);
}

int h263mi_mixed_decode_next_pictures(h263mi_mixed *m, uint32_t decoder_options, const uint8_t *const *data, const size_t *len,
                                      size_t *consumed, uint32_t n_threads, int *stream_rc, uint8_t strength,
                                      uint8_t *const *d_rgba, const size_t *rgba_capacity, h263mi_picture_desc *descs)
{
    return h263mi_mixed_decode_next_pictures_ps(m, decoder_options, data, len, consumed, n_threads, stream_rc, strength, nullptr, d_rgba,
                                                rgba_capacity, descs);
}

int h263mi_mixed_decode_next_pictures_ps(h263mi_mixed *m, uint32_t decoder_options, const uint8_t *const *data, const size_t *len,
                                         size_t *consumed, uint32_t n_threads, int *stream_rc, uint8_t strength,
                                         const uint8_t *strengths, uint8_t *const *d_rgba, const size_t *rgba_capacity,
                                         h263mi_picture_desc *descs)
{
    if (!m || !data || !len || !stream_rc || (d_rgba && !rgba_capacity)) return H263MI_ERR_INVALID_ARGUMENT;
    const uint32_t n = m->n;
    // the strength of every stream's picture: the caller's (one for all, or one per stream of the set), or what the picture's
    // own header asks for (filled in per class below, once the headers have been parsed)
    h263mi_batch::Strengths set_strength;
    RC_TRY(make_strengths(strength, strengths, n, /*from_header_allowed=*/true, set_strength));
    const bool from_header = !strengths && strength == H263MI_STRENGTH_FROM_HEADER;
    for (uint32_t i = 0; i < n; i++)
        if (!data[i] && len[i]) return H263MI_ERR_INVALID_ARGUMENT;
    DeviceGuard g(m->cfg.device_id);
    if (!g.ok) return H263MI_ERR_NO_DEVICE;
    // ---- the serial half of decode_next_picture (state.rs:143-427) per stream, on the host threads (the class -- and with
    // it the staging slot -- is known after the header: parsed into the set's own buffers)
    const bool sparse = sparse_records_enabled();
    std::vector<int> rcs(n, H263MI_OK);
    const HostThreadPlan plan = host_thread_plan(n, n_threads);
    parse_streams(plan, [m](unsigned k) -> WorkerPool & { return m->workers(k); }, n, [&](uint32_t i) {
        if (!data[i]) return;
        prepare_for_parse(m->parsed[i], sparse);
        rcs[i] = bits::parse_picture(data[i], len[i], decoder_options, &m->parser_ctx[i], m->parsed[i]);
    });

    // ---- which size each picture has; what must be refused before anything is queued
    std::vector<int> target(n, -1);
    typedef h263mi_mixed::Want Want;
    std::vector<Want> want(n, Want{0, 0});
    for (uint32_t i = 0; i < n; i++) {
        if (consumed) consumed[i] = 0;
        stream_rc[i] = rcs[i];
        if (!data[i] || rcs[i] != H263MI_OK) continue;
        const bits::ParsedPicture &pic = m->parsed[i];
        const uint32_t w = pic.desc.width, h = pic.desc.height;
        int rc = H263MI_OK;
        if (!w || !h || !layout_fits(w, h)) rc = H263MI_ERR_PICTURE_FORMAT_INVALID;
        const bool any_inter = pic.any_inter;       // (the parser's: inter types, macroblocks not coded, macroblocks not reached)
        const int c_old = m->cls[i];
        const bool same = c_old >= 0 && m->classes[c_old].w == w && m->classes[c_old].h == h;
        const h263mi_batch::StreamState *st_old = c_old >= 0 ? &m->classes[c_old].b->ss[m->slot[i]] : nullptr;
        const bool has_ref = st_old && st_old->has_ref && st_old->cur >= 0;
        if (rc == H263MI_OK && any_inter && !has_ref) rc = H263MI_ERR_UNCODED_IFRAME_BLOCKS;          // gather.rs:149
        if (rc == H263MI_OK && any_inter && !same) rc = H263MI_ERR_PICTURE_FORMAT_INVALID;           // (see the head of this section)
        if (rc == H263MI_OK && d_rgba && d_rgba[i] && rgba_capacity[i] < m->rgba_need(w, h)) rc = H263MI_ERR_INVALID_ARGUMENT;
        // (a tensor's base holds whole elements)
        if (rc == H263MI_OK && d_rgba && d_rgba[i] && m->tensored && (uintptr_t)d_rgba[i] % (m->tensor.dtype == H263MI_TENSOR_F32 ? 4u : 2u))
            rc = H263MI_ERR_INVALID_ARGUMENT;
        if (rc == H263MI_OK) {
            want[i] = Want{w, h};
            target[i] = same ? c_old : -2;       // -2: joins a class of that size (existing or new), resolved below
        }
        stream_rc[i] = rc;
    }
    // ---- the joiners of every size: a class with room for them (made, grown, or -- three quarters empty -- shrunk)
    std::vector<int> new_slot(n, -1);            // the slot a joiner is about to take in its target class
    for (uint32_t i = 0; i < n; i++) {
        if (target[i] != -2) continue;
        const uint32_t w = want[i].w, h = want[i].h;
        std::vector<uint32_t> joiners;
        for (uint32_t j = i; j < n; j++)
            if (target[j] == -2 && want[j].w == w && want[j].h == h) joiners.push_back(j);
        int k = m->find_class(w, h);
        // (the picture of a stream that moves away lives in its old slot until the new one's launch is queued: stayers,
        // leavers and joiners all need a slot during this call)
        const uint32_t have = k >= 0 ? m->classes[k].members() : 0u;
        const uint32_t need = have + (uint32_t)joiners.size();
        int rc = H263MI_OK;
        if (k < 0) {
            m->drop_empty_classes(target, want);
            int place = -1;
            for (size_t q = 0; q < m->classes.size(); q++)
                if (!m->classes[q].b) { place = (int)q; break; }
            if (place < 0) { m->classes.push_back(h263mi_mixed::SizeClass()); place = (int)m->classes.size() - 1; }
            m->classes[place].w = w;
            m->classes[place].h = h;
            rc = m->rebuild_class((size_t)place, h263mi_mixed::pow2_at_least(need));
            if (rc != H263MI_OK) m->classes[place] = h263mi_mixed::SizeClass();
            k = place;
        } else if (need > m->classes[k].b->n) {
            rc = m->rebuild_class((size_t)k, h263mi_mixed::pow2_at_least(need));
        }
        for (uint32_t j : joiners) {
            if (rc != H263MI_OK) { target[j] = -1; stream_rc[j] = rc; continue; }
            target[j] = k;
        }
        if (rc != H263MI_OK) continue;
        h263mi_mixed::SizeClass &c = m->classes[k];
        uint32_t s = 0;
        for (uint32_t j : joiners) {
            while (s < c.b->n && c.stream_of_slot[s] >= 0) s++;
            new_slot[j] = (int)s;
            c.stream_of_slot[s] = (int)j;        // (tentative: given back below when the class's launch does not happen)
            s++;
        }
    }
    // (a class that stands three quarters empty gives the room back in h263mi_mixed_sync -- where everything has been waited
    // for anyway -- not here: sizes come out of untrusted bitstreams, and streams that alternate between two sizes could
    // otherwise force a sync, device-to-device copies and an allocation out of every decode call)

    // ---- one launch per class that has pictures
    // (a class whose RENDERING fails does not stop the others: every class that has pictures is decoded, and the first
    // rendering error is what the call returns at the end -- no stream is left with H263MI_OK and no decoded picture)
    int call_rc = H263MI_OK;
    for (size_t k = 0; k < m->classes.size(); k++) {
        h263mi_mixed::SizeClass &c = m->classes[k];
        h263mi_batch *b = c.b;
        c.submitted = false;
        if (!b) continue;                        // (a class that was given up)
        const uint32_t slots = b->n;
        std::vector<const bits::ParsedPicture *> pics(slots, nullptr);
        std::vector<uint8_t *> out_ptrs(slots, nullptr);
        h263mi_batch::Strengths cst;             // ... of this class's slots
        if (from_header || strengths) cst.per_stream.assign(slots, 0);
        else cst.uniform = set_strength.uniform;
        uint32_t members = 0;
        for (uint32_t s = 0; s < slots; s++) {
            const int i = c.stream_of_slot[s];
            if (i < 0 || target[i] != (int)k) continue;
            const bool joins = m->cls[i] != (int)k;
            if (joins ? new_slot[i] != (int)s : m->slot[i] != (int)s) continue;
            pics[s] = &m->parsed[i];
            members++;
            if (d_rgba) out_ptrs[s] = d_rgba[i];
            if (strengths) cst.per_stream[s] = set_strength.of((uint32_t)i);
            // a stream that arrives from another class starts afresh here (it brings an I picture)
            if (joins) b->ss[s] = h263mi_batch::StreamState();
        }
        if (!members) continue;
        const SubmitResult r = submit_parsed(b, pics.data(), plan.threads, sparse, nullptr, std::move(cst), from_header, nullptr, nullptr,
                                             out_ptrs.data());
        c.submitted = r.rc == H263MI_OK;
        for (uint32_t i = 0; i < n; i++) {
            if (target[i] != (int)k) continue;
            if (r.rc != H263MI_OK) {
                // the class's launch did not happen: its members keep their state and get the error, the joiners their old place
                stream_rc[i] = r.rc;
                if (m->cls[i] != (int)k && new_slot[i] >= 0) c.free_slot(new_slot[i]);
                continue;
            }
            // the pictures are decoded: the streams move to this class, their parser state moves on (state.rs:464-483)
            if (m->cls[i] != (int)k) {
                // the slot the stream leaves: given up now, not earlier (its last picture lived there)
                if (m->cls[i] >= 0) m->classes[m->cls[i]].free_slot(m->slot[i]);
                m->cls[i] = (int)k;
                m->slot[i] = new_slot[i];
            }
            m->parser_ctx[i] = m->parsed[i].next;
            if (consumed) consumed[i] = m->parsed[i].bits_consumed / 8;
            if (descs) descs[i] = m->parsed[i].desc;
        }
        if (r.render_rc != H263MI_OK && call_rc == H263MI_OK) call_rc = r.render_rc;
    }
    // a class that is waiting to render its previous pictures and had nothing to decode in this call renders them now
    // (on a pipelined class the rendering rides in the NEXT launch of that class: without one it would wait for the sync)
    for (h263mi_mixed::SizeClass &c : m->classes)
        if (c.b && !c.submitted && c.b->pending.valid) {
            const int rc = c.b->flush_pending();
            if (rc != H263MI_OK && call_rc == H263MI_OK) call_rc = rc;
        }
    return call_rc;
}

int h263mi_mixed_sync(h263mi_mixed *m, int *stream_rc)
{
    if (!m) return H263MI_ERR_INVALID_ARGUMENT;
    DeviceGuard g(m->cfg.device_id);
    if (!g.ok) return H263MI_ERR_NO_DEVICE;
    int first_error = H263MI_OK;
    for (uint32_t i = 0; i < m->n; i++) {
        // (device errors found while a class was rebuilt: delivered here, once)
        if (stream_rc) stream_rc[i] = m->late_rc[i];
        if (m->late_rc[i] != H263MI_OK && first_error == H263MI_OK) first_error = m->late_rc[i];
        m->late_rc[i] = H263MI_OK;
    }
    for (size_t k = 0; k < m->classes.size(); k++) {
        h263mi_mixed::SizeClass &c = m->classes[k];
        if (!c.b) continue;
        std::vector<int> rcs(c.b->n, H263MI_OK);
        const int rc = c.b->sync(rcs.data());
        if (rc != H263MI_OK && first_error == H263MI_OK) first_error = rc;
        for (uint32_t s = 0; s < c.b->n; s++) {
            const int i = c.stream_of_slot[s];
            if (stream_rc && i >= 0 && rcs[s] != H263MI_OK && stream_rc[i] == H263MI_OK) stream_rc[i] = rcs[s];
        }
    }
    // a class that stands three quarters empty gives the room back: everything it had queued has just been waited for, so the
    // rebuild's own sync is free and its device-to-device copies have the device to themselves.  (A failure leaves the class
    // as it was -- roomy, but whole.)
    for (size_t k = 0; k < m->classes.size(); k++) {
        h263mi_mixed::SizeClass &c = m->classes[k];
        if (!c.b || c.b->n < 8) continue;
        const uint32_t mem = c.members();
        if (mem && mem * 4 <= c.b->n) (void)m->rebuild_class(k, h263mi_mixed::pow2_at_least(mem));
    }
    return first_error;
}

int h263mi_mixed_copy_yuv(h263mi_mixed *m, uint32_t stream, uint8_t *y, uint8_t *cb, uint8_t *cr)
{
    if (!m || stream >= m->n) return H263MI_ERR_INVALID_ARGUMENT;
    if (m->cls[stream] < 0) return H263MI_ERR_NO_PICTURE;
    DeviceGuard g(m->cfg.device_id);
    return m->classes[m->cls[stream]].b->copy_yuv((uint32_t)m->slot[stream], y, cb, cr);
}

int h263mi_mixed_digest_yuv(h263mi_mixed *m, uint32_t seed, uint32_t *digests, int *stream_rc)
{
    if (!m || !digests || !digest_seed_valid(seed)) return H263MI_ERR_INVALID_ARGUMENT;
    DeviceGuard g(m->cfg.device_id);
    for (uint32_t i = 0; i < m->n; i++) {
        digests[i] = 0;
        if (stream_rc) stream_rc[i] = H263MI_ERR_NO_PICTURE;
    }
    // one launch pair per size class that has pictures; a slot nobody sits in digests nothing (its stream state is empty)
    bool missing = false;
    std::vector<uint32_t> of_slot;
    std::vector<int> rc_of_slot;
    for (h263mi_mixed::SizeClass &c : m->classes) {
        if (!c.b || !c.b->any_picture()) continue;
        of_slot.assign(c.b->n, 0u);
        rc_of_slot.assign(c.b->n, H263MI_OK);
        RC_TRY(digest_rc(c.b->digest_yuv(seed, of_slot.data(), rc_of_slot.data())));
        for (uint32_t s = 0; s < c.b->n; s++) {
            const int i = c.stream_of_slot[s];
            if (i < 0 || m->cls[i] < 0 || &m->classes[m->cls[i]] != &c || m->slot[i] != (int)s) continue;
            digests[i] = of_slot[s];
            if (stream_rc) stream_rc[i] = rc_of_slot[s];
        }
    }
    for (uint32_t i = 0; i < m->n; i++) {
        const bool has = m->cls[i] >= 0 && m->classes[m->cls[i]].b && m->classes[m->cls[i]].b->ss[m->slot[i]].cur >= 0;
        if (!has) {
            missing = true;
            digests[i] = 0;
            if (stream_rc) stream_rc[i] = H263MI_ERR_NO_PICTURE;
        }
    }
    return missing && !stream_rc ? H263MI_ERR_NO_PICTURE : H263MI_OK;
}

int h263mi_mixed_reset_stream(h263mi_mixed *m, uint32_t stream)
{
    if (!m || stream >= m->n) return H263MI_ERR_INVALID_ARGUMENT;
    DeviceGuard g(m->cfg.device_id);
    if (!g.ok) return H263MI_ERR_NO_DEVICE;
    int rc = H263MI_OK;
    if (m->cls[stream] >= 0) {
        h263mi_mixed::SizeClass &c = m->classes[m->cls[stream]];
        rc = c.b->forget_stream((uint32_t)m->slot[stream]);
        c.stream_of_slot[m->slot[stream]] = -1;          // the stream leaves its class: the slot is free
    }
    m->cls[stream] = -1;
    m->slot[stream] = -1;
    m->late_rc[stream] = H263MI_OK;
    m->parser_ctx[stream] = bits::ParserContext();
    return rc;
}

}  // extern "C"
