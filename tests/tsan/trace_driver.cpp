// tests/tsan/trace_driver.cpp -- the LAUNCH TRACE of the library's host path: which kernels a call launches, on which stream, from
// and to which memory, with which arguments, behind which events.
//
// Built with g++ -fsanitize=address,undefined from the product's host sources against the stub runtime (stub_runtime.cpp has the
// recorder and the format of its lines); C ABI only.  The stub computes nothing, so the pictures' content does not matter --
// zeroed device records, and bitstreams of flat grey where an entry parses -- and what the trace shows is the host's decisions
// alone.  tests/test_launch_trace.py compares the output byte for byte with tests/golden/launch_trace.txt, which was recorded
// before the output shapes moved out of batch.cpp: a change of the host sources that is meant to change no behaviour changes no
// line of it.
//
// Batches of 3 streams of 48 x 32 (3 x 2 macroblocks) decode one I and two P pictures:
//   batch kind   plain, H263MI_CFG_PIPELINE_POST, H263MI_CFG_OVERLAP_POST
//   shape        the nine of kShapes: default; RGBA layout, resize, resize that is a layout; YUV layouts on the wide and on the
//                narrow path; YUV resize, resize that is a layout; an RGBA and a YUV resize together
//   streams      all active, or stream 1 inactive               } plain batches only: the other kinds take the first of each
//   strength     one for all, or one per stream                 } (the golden stays below the largest fixture of tests/golden)
// and on top of that: a shape switched while a pipelined rendering is pending, h263mi_batch_render_rgba_ps behind the decodes,
// the shaped h263mi_render_* entries of a state, and a mixed-size set (3 streams of 48 x 32, one of 32 x 32) under
// h263mi_mixed_set_rgba_resize.
// usage: trace_driver <output file>; exit code 0 = every call returned what it should and nothing is left allocated
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
static void expect(const char *what, int line, int rc, int want)
{
    if (rc == want) return;
    fprintf(stderr, "trace_driver: line %d: %s returned %d, expected %d\n", line, what, rc, want);
    g_bad++;
}
#define OK(call) expect(#call, __LINE__, (call), H263MI_OK)

static const uint16_t W = 48, H = 32, W2 = 32, H2 = 32;
static const uint32_t N = 3;
// the caller's output: one allocation, the RGBA at its start and the planes behind it
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

// ---- the shapes
static const uint64_t kRgbaOffsets[N] = {4096, 0, 2048};
static const uint64_t kOffsetsY[N] = {0, 4096, 8192}, kOffsetsC[N] = {2048, 6144, 10240};

static void rgba_resize(h263mi_batch *b, uint16_t ow, uint16_t oh, uint64_t pitch)
{
    h263mi_rgba_resize r{};
    r.out_width = ow;
    r.out_height = oh;
    r.row_pitch = pitch;
    OK(h263mi_batch_set_rgba_resize(b, &r));
}
static void yuv_layout(h263mi_batch *b, uint8_t format, uint64_t pitch_y, uint64_t pitch_c, bool offsets)
{
    h263mi_yuv_layout l{};
    l.format = format;
    l.pitch_y = pitch_y;
    l.pitch_c = pitch_c;
    l.offsets_y = offsets ? kOffsetsY : nullptr;
    l.offsets_cb = offsets ? kOffsetsC : nullptr;
    OK(h263mi_batch_set_yuv_layout(b, &l));
}
static void yuv_resize(h263mi_batch *b, uint16_t ow, uint16_t oh, uint8_t format, uint64_t pitch_y, uint64_t pitch_c)
{
    h263mi_yuv_resize r{};
    r.out_width = ow;
    r.out_height = oh;
    r.format = format;
    r.pitch_y = pitch_y;
    r.pitch_c = pitch_c;
    OK(h263mi_batch_set_yuv_resize(b, &r));
}
struct Shape {
    const char *name;
    bool planes;                 // the picture in the middle renders planes alone (else RGBA alone); the others render both
    void (*set)(h263mi_batch *b);
};
// default; RGBA at half size with rows 128 bytes apart and explicit offsets; RGBA resized to 20 x 12 (needs the scratch) and to
// 24 x 16 (is the half-size layout); NV12 with offsets, all multiples of 4 (the wide stores); I420 at pitches 50 and 25 (the narrow
// path); I420 resized to 20 x 12 and to 48 x 32 (is the layout); RGBA and NV12 both resized to 20 x 12
static const Shape kShapes[] = {
    {"default", false, [](h263mi_batch *) {}},
    {"rgba layout", false, [](h263mi_batch *b) {
         h263mi_rgba_layout l{};
         l.scale_log2 = 1;
         l.row_pitch = 128;
         l.offsets = kRgbaOffsets;
         OK(h263mi_batch_set_rgba_layout(b, &l));
     }},
    {"rgba resize", false, [](h263mi_batch *b) { rgba_resize(b, 20, 12, 96); }},
    {"rgba resize=layout", false, [](h263mi_batch *b) { rgba_resize(b, 24, 16, 0); }},
    {"yuv nv12 wide", true, [](h263mi_batch *b) { yuv_layout(b, H263MI_YUV_NV12, 64, 64, true); }},
    {"yuv i420 narrow", true, [](h263mi_batch *b) { yuv_layout(b, H263MI_YUV_I420, 50, 25, false); }},
    {"yuv resize", true, [](h263mi_batch *b) { yuv_resize(b, 20, 12, H263MI_YUV_I420, 0, 0); }},
    {"yuv resize=layout", true, [](h263mi_batch *b) { yuv_resize(b, 48, 32, H263MI_YUV_I420, 64, 32); }},
    {"rgba+yuv resize", true, [](h263mi_batch *b) {
         rgba_resize(b, 20, 12, 0);
         yuv_resize(b, 20, 12, H263MI_YUV_NV12, 32, 32);
     }},
};
static const size_t kNShapes = sizeof kShapes / sizeof kShapes[0];
static const char *const kKindNames[] = {"plain", "pipeline", "overlap"};
static const uint32_t kKindFlags[] = {0, H263MI_CFG_PIPELINE_POST, H263MI_CFG_OVERLAP_POST};
static const uint8_t kStrengths[N] = {0, 7, 12};

// one batch of a kind, with zeroed records and the caller's output buffer
struct Batch {
    h263mi_batch *b = nullptr;
    DeviceBuffer records, out;
    explicit Batch(int kind) : records((size_t)N * 6 * sizeof(h263mi_mb_record), false), out(kOutBytes, true)
    {
        h263mi_backend_cfg cfg{0, kKindFlags[kind], nullptr};
        OK(h263mi_batch_create(N, W, H, &cfg, &b));
    }
    ~Batch() { h263mi_batch_destroy(b); }
    // want: 1 RGBA, 2 planes, 3 both
    void decode(uint8_t type, bool per_stream, int want)
    {
        OK(h263mi_batch_decode_ps(b, type, static_cast<const h263mi_mb_record *>(records.p), nullptr, nullptr, 0, 5,
                                  per_stream ? kStrengths : nullptr, (want & 1) ? out.at(0) : nullptr, (want & 2) ? out.at(kPlanesAt) : nullptr));
    }
    void decode_three(const Shape &shape, bool per_stream)
    {
        decode(H263MI_PICTURE_I, per_stream, 3);
        decode(H263MI_PICTURE_P, per_stream, shape.planes ? 2 : 1);
        decode(H263MI_PICTURE_P, per_stream, 3);
    }
};

static void run_batch(int kind, const Shape &shape, bool inactive, bool per_stream)
{
    const std::string title = std::string("batch ") + kKindNames[kind] + " | " + shape.name + " | " + (inactive ? "stream 1 inactive" : "all") +
                              " | " + (per_stream ? "strengths" : "strength");
    stub_trace_section(title.c_str());
    Batch t(kind);
    if (!t.b) return;
    shape.set(t.b);
    const uint8_t active[N] = {1, 0, 1};
    if (inactive) OK(h263mi_batch_set_active(t.b, active));
    t.decode_three(shape, per_stream);
    OK(h263mi_batch_sync(t.b));
}

// the shape of a pipelined batch changes while a rendering waits for the next launch: the rendering keeps the shape of its request
static void run_switch_while_pending()
{
    stub_trace_section("pipeline | shapes switched while a rendering is pending");
    Batch t(1);
    if (!t.b) return;
    kShapes[8].set(t.b);
    t.decode(H263MI_PICTURE_I, false, 3);
    OK(h263mi_batch_set_rgba_layout(t.b, nullptr));
    kShapes[4].set(t.b);
    t.decode(H263MI_PICTURE_P, false, 3);
    kShapes[3].set(t.b);
    OK(h263mi_batch_set_yuv_resize(t.b, nullptr));
    t.decode(H263MI_PICTURE_P, true, 3);
    kShapes[2].set(t.b);
    OK(h263mi_batch_sync(t.b));
}

// h263mi_batch_render_rgba_ps behind the decodes: every stream's last picture, with a stream that has none
static void run_render(int kind, const Shape &shape)
{
    const std::string title = std::string("render ") + kKindNames[kind] + " | " + shape.name;
    stub_trace_section(title.c_str());
    Batch t(kind);
    if (!t.b) return;
    shape.set(t.b);
    t.decode(H263MI_PICTURE_I, false, 0);
    t.decode(H263MI_PICTURE_P, false, 3);
    OK(h263mi_batch_render_rgba_ps(t.b, 0, kStrengths, t.out.at(0), t.out.at(kPlanesAt)));
    OK(h263mi_batch_reset_stream(t.b, 1));
    OK(h263mi_batch_render_rgba_ps(t.b, 9, nullptr, t.out.at(0), nullptr));
    OK(h263mi_batch_render_rgba_ps(t.b, 9, nullptr, nullptr, t.out.at(kPlanesAt)));
    OK(h263mi_batch_sync(t.b));
}

// ---- coded pictures of flat grey for the entries that parse: Sorenson Spark, version 1, an 8-bit custom size
struct BitWriter {
    std::vector<uint8_t> bytes;
    unsigned n = 0;
    void put(uint32_t value, unsigned bits)
    {
        for (unsigned i = bits; i-- > 0; n++) {
            if (n % 8 == 0) bytes.push_back(0);
            bytes.back() = (uint8_t)(bytes.back() | (((value >> i) & 1u) << (7 - n % 8)));
        }
    }
};
static std::vector<uint8_t> coded_picture(uint16_t w, uint16_t h, uint8_t type, uint8_t temporal_reference)
{
    BitWriter bw;
    bw.put(1, 17);                       // start code
    bw.put(1, 5);                        // version
    bw.put(temporal_reference, 8);
    bw.put(0, 3);                        // the size follows in 8 bits each
    bw.put(w, 8);
    bw.put(h, 8);
    bw.put(type, 2);
    bw.put(1, 1);                        // deblocking asked for
    bw.put(8, 5);                        // quantiser
    bw.put(0, 1);                        // no extra information
    const unsigned mbs = (unsigned)((w + 15) / 16) * ((h + 15) / 16);
    for (unsigned m = 0; m < mbs; m++) {
        if (type != H263MI_PICTURE_I) {
            bw.put(1, 1);                // COD: not coded
            continue;
        }
        bw.put(1, 1);                    // MCBPC: INTRA, no coded chroma block
        bw.put(3, 4);                    // CBPY: no coded luma block
        for (int blk = 0; blk < 6; blk++) bw.put(64, 8);       // INTRADC
    }
    return bw.bytes;
}

// the four shaped rendering entries of a state (and the unshaped one), each in a form that is a layout and one that is not
static void run_state()
{
    stub_trace_section("state | h263mi_render_rgba_layout, _rgba_resize, _yuv, _yuv_resize");
    h263mi_state *st = nullptr;
    OK(h263mi_state_new(H263MI_SORENSON_SPARK_BITSTREAM, nullptr, &st));
    if (!st) return;
    for (uint8_t k = 0; k < 2; k++) {
        const std::vector<uint8_t> pic = coded_picture(W, H, k ? H263MI_PICTURE_P : H263MI_PICTURE_I, k);
        OK(h263mi_decode_next_picture(st, pic.data(), pic.size(), nullptr));
    }
    std::vector<uint8_t> host(16384);
    OK(h263mi_render_rgba(st, H263MI_STRENGTH_FROM_HEADER, host.data()));
    h263mi_rgba_layout l{};
    OK(h263mi_render_rgba_layout(st, 3, &l, host.data()));
    l.scale_log2 = 1;
    l.row_pitch = 128;
    OK(h263mi_render_rgba_layout(st, 3, &l, host.data()));
    h263mi_rgba_resize r{};
    r.out_width = 20, r.out_height = 12, r.row_pitch = 96;
    OK(h263mi_render_rgba_resize(st, H263MI_STRENGTH_FROM_HEADER, &r, host.data()));
    r.out_width = 12, r.out_height = 8, r.row_pitch = 0;                      // (the 1/4 layout)
    OK(h263mi_render_rgba_resize(st, 0, &r, host.data()));
    OK(h263mi_render_yuv(st, 4, nullptr, host.data()));
    const uint64_t off_y = 1000, off_cb = 8500, off_cr = 0;
    h263mi_yuv_layout y{};
    y.format = H263MI_YUV_NV12;
    y.pitch_y = 100;
    y.pitch_c = 50;
    y.offsets_y = &off_y, y.offsets_cb = &off_cb;
    OK(h263mi_render_yuv(st, 4, &y, host.data()));
    h263mi_yuv_resize yr{};
    yr.out_width = 20, yr.out_height = 12, yr.format = H263MI_YUV_I420;
    yr.pitch_y = 33, yr.pitch_c = 17;
    yr.offsets_y = &off_y, yr.offsets_cb = &off_cb, yr.offsets_cr = &off_cr;
    OK(h263mi_render_yuv_resize(st, H263MI_STRENGTH_FROM_HEADER, &yr, host.data()));
    yr.format = H263MI_YUV_NV12;
    yr.pitch_c = 34;
    yr.offsets_cr = nullptr;
    OK(h263mi_render_yuv_resize(st, 2, &yr, host.data()));
    yr.out_width = W, yr.out_height = H, yr.pitch_y = 100, yr.pitch_c = 50;  // (the full-size layout)
    OK(h263mi_render_yuv_resize(st, 2, &yr, host.data()));
    h263mi_state_free(st);
}

// a mixed-size set under h263mi_mixed_set_rgba_resize: for one class the resize is a layout, for the other it is not
static void run_mixed(bool pipeline)
{
    stub_trace_section(pipeline ? "mixed set, pipeline | h263mi_mixed_set_rgba_resize" : "mixed set | h263mi_mixed_set_rgba_resize");
    const uint32_t n = 4;
    h263mi_backend_cfg cfg{0, pipeline ? H263MI_CFG_PIPELINE_POST : 0u, nullptr};
    h263mi_mixed *m = nullptr;
    OK(h263mi_mixed_create(n, &cfg, &m));
    if (!m) return;
    {
        DeviceBuffer out(kOutBytes, true);
        uint8_t *bufs[n];
        size_t caps[n];
        for (uint32_t s = 0; s < n; s++) {
            bufs[s] = out.at((size_t)s * 8192);
            caps[s] = (size_t)W * H * 4;
        }
        uint8_t tr = 0;
        auto decode = [&](uint8_t type, bool skip_stream_2, const uint8_t *strengths) {
            const std::vector<uint8_t> big = coded_picture(W, H, type, tr), small = coded_picture(W2, H2, type, tr);
            tr++;
            const uint8_t *data[n] = {big.data(), big.data(), skip_stream_2 ? nullptr : big.data(), small.data()};
            const size_t len[n] = {big.size(), big.size(), skip_stream_2 ? 0 : big.size(), small.size()};
            size_t used[n] = {0, 0, 0, 0};
            int rcs[n] = {-1, -1, -1, -1};
            OK(h263mi_mixed_decode_next_pictures_ps(m, H263MI_SORENSON_SPARK_BITSTREAM, data, len, used, 1, rcs,
                                                    strengths ? 0 : H263MI_STRENGTH_FROM_HEADER, strengths, bufs, caps, nullptr));
            for (uint32_t s = 0; s < n; s++)
                if (data[s]) OK(rcs[s]);
        };
        const uint8_t strengths[n] = {1, 2, 3, 4};
        decode(H263MI_PICTURE_I, false, nullptr);
        h263mi_rgba_resize r{};
        r.out_width = 20, r.out_height = 12, r.row_pitch = 96;
        OK(h263mi_mixed_set_rgba_resize(m, &r));
        decode(H263MI_PICTURE_P, false, nullptr);
        r.out_width = 24, r.out_height = 16, r.row_pitch = 0;                 // (48 x 32: the 1/2 layout; 32 x 32: a resize)
        OK(h263mi_mixed_set_rgba_resize(m, &r));
        decode(H263MI_PICTURE_P, true, strengths);
        decode(H263MI_PICTURE_P, false, nullptr);
        OK(h263mi_mixed_set_rgba_resize(m, nullptr));
        decode(H263MI_PICTURE_P, false, strengths);
        OK(h263mi_mixed_sync(m, nullptr));
        h263mi_mixed_destroy(m);
    }
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: trace_driver <output file>\n");
        return 2;
    }
    std::string trace;
    stub_trace_into(&trace);
    for (int kind = 0; kind < 3; kind++)
        for (size_t shape = 0; shape < kNShapes; shape++)
            for (int inactive = 0; inactive < (kind == 0 ? 2 : 1); inactive++)
                for (int per_stream = 0; per_stream < (kind == 0 ? 2 : 1); per_stream++)
                    run_batch(kind, kShapes[shape], inactive != 0, per_stream != 0);
    run_switch_while_pending();
    for (int kind = 0; kind < 3; kind++)
        for (size_t shape : {(size_t)0, (size_t)8})
            if (kind == 0 || shape) run_render(kind, kShapes[shape]);
    run_state();
    for (bool pipeline : {false, true}) run_mixed(pipeline);
    stub_trace_into(nullptr);
    if (stub_live_allocations() != 0) {
        fprintf(stderr, "trace_driver: %ld allocations, events or streams are left\n", stub_live_allocations());
        g_bad++;
    }
    FILE *f = fopen(argv[1], "wb");
    if (!f || fwrite(trace.data(), 1, trace.size(), f) != trace.size() || fclose(f) != 0) {
        fprintf(stderr, "trace_driver: cannot write %s\n", argv[1]);
        return 2;
    }
    return g_bad ? 1 : 0;
}
