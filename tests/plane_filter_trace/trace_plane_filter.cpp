// trace_plane_filter.cpp -- the launch trace of the host path of a FILTERED YUV resize (h263mi_batch_set_yuv_resize_filtered,
// h263mi_render_yuv_resize_filtered), in the manner of tests/tsan/trace_driver.cpp (TEST INFRASTRUCTURE).
//
// Built by tests/test_plane_filter_trace.py with g++ -fsanitize=address,undefined from the product's host sources against
// stub_with_plane_filter.cpp; C ABI only; a stand-alone program.  Batches of 3 streams of 48 x 32 with zeroed records; the
// sections are named, and the test compares them with one another and with what the definition says.
// usage: trace_plane_filter <output file>; exit code 0 = every call returned what it should and nothing is left allocated
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/h263mi.h"

long stub_live_allocations();                        // stub_runtime.cpp
void stub_trace_into(std::string *sink);
void stub_trace_section(const char *title);
void stub_trace_output(const void *p);

static int g_bad = 0;
static void expect(const char *what, int line, long rc, long want)
{
    if (rc == want) return;
    fprintf(stderr, "trace_plane_filter: line %d: %s is %ld, expected %ld\n", line, what, rc, want);
    g_bad++;
}
#define OK(call) expect(#call, __LINE__, (call), H263MI_OK)
#define REFUSED(call) expect(#call, __LINE__, (call), H263MI_ERR_INVALID_ARGUMENT)

static const uint16_t W = 48, H = 32;
static const uint32_t N = 3;
static const size_t kPlanesAt = 20480, kOutBytes = 32768;

struct DeviceBuffer {
    void *p = nullptr;
    DeviceBuffer(size_t bytes, bool output)
    {
        OK(h263mi_device_malloc(0, bytes, &p));
        const std::vector<uint8_t> zero(bytes, 0);
        OK(h263mi_device_memcpy_h2d(0, p, zero.data(), bytes));
        if (output) stub_trace_output(p);
    }
    ~DeviceBuffer() { OK(h263mi_device_free(0, p)); }
    uint8_t *at(size_t off) const { return static_cast<uint8_t *>(p) + off; }
};

static h263mi_yuv_resize resize_of(uint16_t ow, uint16_t oh, uint8_t format, uint64_t pitch_y, uint64_t pitch_c)
{
    h263mi_yuv_resize r{};
    r.out_width = ow, r.out_height = oh, r.format = format, r.pitch_y = pitch_y, r.pitch_c = pitch_c;
    return r;
}
static h263mi_filter filter_of(uint8_t kind)
{
    h263mi_filter f{};
    f.kind = kind;
    return f;
}

struct Batch {
    h263mi_batch *b = nullptr;
    DeviceBuffer records, out;
    explicit Batch(uint32_t flags) : records((size_t)N * 6 * sizeof(h263mi_mb_record), false), out(kOutBytes, true)
    {
        h263mi_backend_cfg cfg{0, flags, nullptr};
        OK(h263mi_batch_create(N, W, H, &cfg, &b));
    }
    ~Batch() { h263mi_batch_destroy(b); }
    // want: 1 RGBA, 2 planes, 3 both
    void decode(uint8_t type, int want)
    {
        OK(h263mi_batch_decode_ps(b, type, static_cast<const h263mi_mb_record *>(records.p), nullptr, nullptr, 0, 5, nullptr,
                                  (want & 1) ? out.at(0) : nullptr, (want & 2) ? out.at(kPlanesAt) : nullptr));
    }
    void render(int want)
    {
        OK(h263mi_batch_render_rgba_ps(b, 7, nullptr, (want & 1) ? out.at(0) : nullptr, (want & 2) ? out.at(kPlanesAt) : nullptr));
    }
};

// one plain batch under the YUV shape that `set` makes: a decode that renders RGBA and planes, a rendering of the planes alone
template <typename Set>
static void run_shape(const char *title, Set set)
{
    stub_trace_section(title);
    Batch t(0);
    if (!t.b) return;
    set(t.b);
    t.decode(H263MI_PICTURE_I, 3);
    t.render(2);
    OK(h263mi_batch_sync(t.b));
}

// the setter makes the scratch and the tables, once: two allocations at the setter, none at any later rendering
static void run_tables_once()
{
    stub_trace_section("filtered | tables made once");
    Batch t(0);
    if (!t.b) return;
    const h263mi_yuv_resize r = resize_of(20, 12, H263MI_YUV_I420, 0, 0);
    const h263mi_filter f = filter_of(H263MI_FILTER_BICUBIC);
    const long before = stub_live_allocations();
    OK(h263mi_batch_set_yuv_resize_filtered(t.b, &r, &f));
    expect("allocations made by the setter", __LINE__, stub_live_allocations() - before, 2);
    t.decode(H263MI_PICTURE_I, 2);
    t.render(2);                                     // (the rings of the uploads are made by now)
    const long warm = stub_live_allocations();
    t.render(2);
    t.decode(H263MI_PICTURE_P, 3);
    t.render(3);
    expect("allocations made by later renderings", __LINE__, stub_live_allocations() - warm, 0);
    // the same shape set again: new scratch and tables, the old ones freed
    OK(h263mi_batch_set_yuv_resize_filtered(t.b, &r, &f));
    expect("allocations after the shape was set again", __LINE__, stub_live_allocations() - warm, 0);
    OK(h263mi_batch_set_yuv_resize_filtered(t.b, nullptr, &f));
    expect("allocations after the default was restored", __LINE__, stub_live_allocations() - warm, -2);
    OK(h263mi_batch_sync(t.b));
}

// a refused filter leaves the shape in force untouched: the same rendering before and after
static void run_refusals()
{
    Batch t(0);
    if (!t.b) return;
    const h263mi_yuv_resize r = resize_of(20, 12, H263MI_YUV_NV12, 32, 32), other = resize_of(9, 9, H263MI_YUV_I420, 0, 0);
    const h263mi_filter good = filter_of(H263MI_FILTER_BILINEAR);
    OK(h263mi_batch_set_yuv_resize_filtered(t.b, &r, &good));
    t.decode(H263MI_PICTURE_I, 0);
    OK(h263mi_batch_sync(t.b));
    stub_trace_section("refusals | before");
    t.render(2);
    OK(h263mi_batch_sync(t.b));
    h263mi_filter bad_kind = filter_of(3), bad_reserved = filter_of(H263MI_FILTER_BICUBIC);
    bad_reserved.reserved[4] = 1;
    const long live = stub_live_allocations();
    REFUSED(h263mi_batch_set_yuv_resize_filtered(t.b, &other, &bad_kind));
    REFUSED(h263mi_batch_set_yuv_resize_filtered(t.b, &other, &bad_reserved));
    REFUSED(h263mi_batch_set_yuv_resize_filtered(t.b, nullptr, &bad_kind));
    h263mi_yuv_resize zero = other;
    zero.out_width = 0;
    REFUSED(h263mi_batch_set_yuv_resize_filtered(t.b, &zero, &good));
    expect("allocations made by refused setters", __LINE__, stub_live_allocations() - live, 0);
    stub_trace_section("refusals | after");
    t.render(2);
    OK(h263mi_batch_sync(t.b));
}

// the shape of a pipelined batch changes while a rendering waits for the next launch: the rendering keeps the filter, the scratch
// and the tables of its request (AddressSanitizer sees a table or a scratch that was freed too early)
static void run_switch_while_pending()
{
    stub_trace_section("pipeline | shape switched while a filtered rendering is pending");
    Batch t(H263MI_CFG_PIPELINE_POST);
    if (!t.b) return;
    const h263mi_yuv_resize r = resize_of(20, 12, H263MI_YUV_I420, 0, 0), small = resize_of(10, 6, H263MI_YUV_I420, 0, 0);
    const h263mi_filter cubic = filter_of(H263MI_FILTER_BICUBIC), area = filter_of(H263MI_FILTER_AREA);
    OK(h263mi_batch_set_yuv_resize_filtered(t.b, &r, &cubic));
    t.decode(H263MI_PICTURE_I, 2);                   // deferred
    OK(h263mi_batch_set_yuv_resize_filtered(t.b, &small, &area));
    t.decode(H263MI_PICTURE_P, 2);                   // k_frame renders the first request: filtered
    OK(h263mi_batch_set_yuv_resize_filtered(t.b, &r, &cubic));
    t.decode(H263MI_PICTURE_P, 2);                   // ... the second: the area average
    OK(h263mi_batch_set_yuv_resize(t.b, nullptr));
    OK(h263mi_batch_sync(t.b));                      // flush_pending renders the third: filtered again
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: trace_plane_filter <output file>\n");
        return 2;
    }
    std::string trace;
    stub_trace_into(&trace);
    static const h263mi_yuv_resize small = resize_of(20, 12, H263MI_YUV_I420, 0, 0), full = resize_of(W, H, H263MI_YUV_I420, 64, 32);
    static const h263mi_filter cubic = filter_of(H263MI_FILTER_BICUBIC), linear = filter_of(H263MI_FILTER_BILINEAR), area = filter_of(H263MI_FILTER_AREA);
    run_shape("shape | bicubic", [](h263mi_batch *b) { OK(h263mi_batch_set_yuv_resize_filtered(b, &small, &cubic)); });
    run_shape("shape | bilinear", [](h263mi_batch *b) { OK(h263mi_batch_set_yuv_resize_filtered(b, &small, &linear)); });
    run_shape("shape | unfiltered", [](h263mi_batch *b) { OK(h263mi_batch_set_yuv_resize(b, &small)); });
    run_shape("shape | area", [](h263mi_batch *b) { OK(h263mi_batch_set_yuv_resize_filtered(b, &small, &area)); });
    run_shape("shape | null", [](h263mi_batch *b) { OK(h263mi_batch_set_yuv_resize_filtered(b, &small, nullptr)); });
    run_shape("shape | layout", [](h263mi_batch *b) {
        h263mi_yuv_layout l{};
        l.format = H263MI_YUV_I420, l.pitch_y = 64, l.pitch_c = 32;
        OK(h263mi_batch_set_yuv_layout(b, &l));
    });
    run_shape("shape | full size bicubic", [](h263mi_batch *b) { OK(h263mi_batch_set_yuv_resize_filtered(b, &full, &cubic)); });
    // a filtered shape replaces a layout and is replaced by a resize
    run_shape("shape | layout, then bicubic", [](h263mi_batch *b) {
        h263mi_yuv_layout l{};
        l.format = H263MI_YUV_NV12;
        OK(h263mi_batch_set_yuv_layout(b, &l));
        OK(h263mi_batch_set_yuv_resize_filtered(b, &small, &cubic));
    });
    run_shape("shape | bicubic, then unfiltered", [](h263mi_batch *b) {
        OK(h263mi_batch_set_yuv_resize_filtered(b, &small, &cubic));
        OK(h263mi_batch_set_yuv_resize(b, &small));
    });
    run_tables_once();
    run_refusals();
    run_switch_while_pending();
    stub_trace_into(nullptr);
    if (stub_live_allocations() != 0) {
        fprintf(stderr, "trace_plane_filter: %ld allocations, events or streams are left\n", stub_live_allocations());
        g_bad++;
    }
    FILE *f = fopen(argv[1], "wb");
    if (!f || fwrite(trace.data(), 1, trace.size(), f) != trace.size() || fclose(f) != 0) {
        fprintf(stderr, "trace_plane_filter: cannot write %s\n", argv[1]);
        return 2;
    }
    return g_bad ? 1 : 0;
}
