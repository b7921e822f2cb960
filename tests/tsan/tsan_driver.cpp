// tests/tsan/tsan_driver.cpp -- the host pipeline of libh263mi under ThreadSanitizer.
//
// Built with g++ -fsanitize=thread from the PRODUCT's host sources (worker_pool.cpp, batch.cpp, output_shape.cpp, batch_staging.cpp,
// mixed_set.cpp, state.cpp, device_util.cpp, host/bitstream.cpp) against a stub of the HIP runtime (hip_stub/, plain malloc
// for device and pinned memory, stub kernel launchers): what runs here is the real WorkerPool (spin-then-park, generation
// word), the real stream-affinity / stealing deal, the real parser writing records, events, block offsets and the group index
// of N streams straight into one pinned staging slot at per-stream pitches, and the real enqueue path that reads the slot.
// The reference needs none of this: it is single-threaded safe Rust (`&mut self`, state.rs:138-141).
//
// Scenarios (all through the C ABI):
//   * one batch, calls back to back with 1 .. 40 parser threads, random NULL streams, random pauses between the calls so that
//     the workers are met spinning, about to park and parked; under a fake 2-CPU quota (H263MI_CGROUP_CPU_MAX) so that calls
//     with more threads than the quota take the parking plan (spin 0) and the others the spinning plan;
//   * pools torn down in the middle of an idle spin and right after a call;
//   * two batches, a mixed-size set and one H263State driven from four threads at the same time (distinct objects may be);
//   * with a second corpus of another size: streams of the mixed-size set that move between the two classes at key frames, a P
//     picture of the other size refused, a class that doubles when streams join it and shrinks at the sync that finds it at most
//     a quarter full;
//   * the packed (H263MI_DIRECT_WORDS=0) transport, and workers that never park (H263MI_SPIN_US = 50 ms, no quota, at most 6
//     threads: every hand-over goes through the generation word alone, never through the mutex): further runs of the test.
//   * a failure injected at every HIP call of h263mi_submit_picture[_events], h263mi_decode_next_picture, a 2-stream
//     h263mi_batch_submit_host and h263mi_batch_decode_next_pictures_ps, and of the shaped h263mi_render_* entries of a state: the
//     last picture stays as it was; of h263mi_batch_set_rgba_resize, _set_yuv_layout and _set_yuv_resize: the shape that was in
//     force stays in force (the launch trace of a rendering, stub_runtime.cpp, is what it was); and of a 3-stream,
//     two-size h263mi_mixed_decode_next_pictures_ps in which a stream moves class; every pinned block, device block and event
//     the objects held is given back (the stub runtime counts them);
//   * the order in which h263mi_submit_picture[_events] names what is wrong with a call, one crafted case per rule.
// Exit code 0 and no ThreadSanitizer report = pass.  The same driver built with -DH263MI_TSAN_BREAK_GENERATION_ORDER (the task is
// published with a relaxed store: worker_pool.cpp) MUST make ThreadSanitizer report a race: tests/test_tsan.py checks both.
// usage: tsan_driver <corpus.bin> [rounds [max threads [corpus2.bin]]]
//   corpus: u32 streams, u32 frames, u32 width, u32 height, then per (stream, frame): u32 length, bytes; corpus2 (optional): the
//   same at another picture size, for the mixed-size set's class moves, growth and shrinking
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <memory>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../../include/h263mi.h"

long stub_live_allocations();                                        // stub_runtime.cpp
void stub_trace_into(std::string *sink);
void stub_trace_output(const void *p);

static std::vector<std::vector<std::vector<uint8_t>>> g_corpus;      // [stream][frame]
static uint16_t g_w, g_h;
// (optional) a second corpus of another picture size: the mixed-size set's second class
static std::vector<std::vector<std::vector<uint8_t>>> g_corpus2;
static uint16_t g_w2, g_h2;
static std::atomic<int> g_failures{0};
static uint32_t g_max_threads = 40;                                  // (third argument: runs whose workers SPIN keep within the CPUs)

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "tsan_driver: %s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            g_failures.fetch_add(1);                                                 \
        }                                                                            \
    } while (0)

static bool load_corpus(const char *path, std::vector<std::vector<std::vector<uint8_t>>> &corpus, uint16_t &w, uint16_t &h)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint32_t hdr[4];
    if (fread(hdr, 4, 4, f) != 4) return false;
    w = (uint16_t)hdr[2];
    h = (uint16_t)hdr[3];
    corpus.assign(hdr[0], std::vector<std::vector<uint8_t>>(hdr[1]));
    for (auto &s : corpus)
        for (auto &p : s) {
            uint32_t n = 0;
            if (fread(&n, 4, 1, f) != 1) return false;
            p.resize(n);
            if (n && fread(p.data(), 1, n, f) != n) return false;
        }
    fclose(f);
    return true;
}

// one batch of `n` streams: every call decodes the next picture of a random subset of them
static void drive_batch(unsigned seed, uint32_t n, int calls, bool pipeline, bool destroy_mid_spin)
{
    std::mt19937 rng(seed);
    h263mi_backend_cfg cfg{0, pipeline ? H263MI_CFG_PIPELINE_POST : 0u, nullptr};
    h263mi_batch *b = nullptr;
    CHECK(h263mi_batch_create(n, g_w, g_h, &cfg, &b) == H263MI_OK);
    if (!b) return;
    void *d_rgba = nullptr;
    CHECK(h263mi_device_malloc(0, (size_t)n * g_w * g_h * 4, &d_rgba) == H263MI_OK);
    std::vector<uint32_t> next(n, 0);
    const uint32_t frames = (uint32_t)g_corpus[0].size();
    static const uint32_t kThreads[] = {1, 2, 3, 5, 8, 13, 16, 24, 40};
    for (int c = 0; c < calls; c++) {
        std::vector<const uint8_t *> data(n, nullptr);
        std::vector<size_t> len(n, 0), used(n, 0);
        std::vector<int> rcs(n, 0);
        uint32_t with_data = 0;
        for (uint32_t s = 0; s < n; s++) {
            const bool key = next[s] == 0;
            if (!key && rng() % 4 == 0) continue;                          // no picture for this stream in this call
            if (next[s] >= frames) next[s] = 0;                            // (the corpus starts every stream with a key frame)
            const std::vector<uint8_t> &p = g_corpus[s % g_corpus.size()][next[s]];
            data[s] = p.data();
            len[s] = p.size();
            with_data++;
        }
        uint32_t threads = kThreads[rng() % (sizeof kThreads / sizeof kThreads[0])];
        if (threads > g_max_threads) threads = 1 + threads % g_max_threads;
        const int rc = h263mi_batch_decode_next_pictures_ex(b, H263MI_SORENSON_SPARK_BITSTREAM, data.data(), len.data(), used.data(),
                                                            threads, rcs.data(), H263MI_STRENGTH_FROM_HEADER, (uint8_t *)d_rgba, nullptr);
        CHECK(rc == H263MI_OK);
        for (uint32_t s = 0; s < n; s++) {
            if (!data[s]) continue;
            CHECK(rcs[s] == H263MI_OK);
            CHECK(used[s] == len[s] || used[s] + 1 == len[s]);      // (whole bytes: the last one may be half padding)
            if (rcs[s] == H263MI_OK) next[s]++;
        }
        if (c % 7 == 6) CHECK(h263mi_batch_sync(b) == H263MI_OK);
        // pauses of 0 .. 700 us: shorter, about as long and longer than the workers' 300 us spin
        const unsigned pause = rng() % 8;
        if (pause) std::this_thread::sleep_for(std::chrono::microseconds(100 * pause));
    }
    if (!destroy_mid_spin) std::this_thread::sleep_for(std::chrono::milliseconds(2));     // everybody parked
    CHECK(h263mi_batch_sync(b) == H263MI_OK);
    h263mi_batch_destroy(b);                                               // (pool teardown: mid-spin or parked)
    CHECK(h263mi_device_free(0, d_rgba) == H263MI_OK);
}

static void drive_mixed(unsigned seed, uint32_t n, int calls)
{
    std::mt19937 rng(seed);
    h263mi_backend_cfg cfg{0, H263MI_CFG_PIPELINE_POST, nullptr};
    h263mi_mixed *m = nullptr;
    CHECK(h263mi_mixed_create(n, &cfg, &m) == H263MI_OK);
    if (!m) return;
    std::vector<void *> bufs(n, nullptr);
    std::vector<size_t> caps(n, (size_t)std::max(g_w * g_h, g_w2 * g_h2) * 4);
    for (uint32_t s = 0; s < n; s++) CHECK(h263mi_device_malloc(0, caps[s], &bufs[s]) == H263MI_OK);
    std::vector<uint32_t> next(n, 0);
    std::vector<uint8_t> small(n, 0);            // the stream's pictures come from the second corpus (moved there at a key frame)
    const uint32_t frames = (uint32_t)g_corpus[0].size();
    for (int c = 0; c < calls; c++) {
        std::vector<const uint8_t *> data(n, nullptr);
        std::vector<size_t> len(n, 0), used(n, 0);
        std::vector<int> rcs(n, 0);
        for (uint32_t s = 0; s < n; s++) {
            if (next[s] && rng() % 3 == 0) continue;
            if (next[s] >= frames) next[s] = 0;
            if (next[s] == 0 && !g_corpus2.empty()) small[s] = rng() % 3 == 0;
            const std::vector<uint8_t> &p = small[s] ? g_corpus2[s % g_corpus2.size()][next[s]] : g_corpus[(s + 3) % g_corpus.size()][next[s]];
            data[s] = p.data();
            len[s] = p.size();
        }
        const int rc = h263mi_mixed_decode_next_pictures(m, H263MI_SORENSON_SPARK_BITSTREAM, data.data(), len.data(), used.data(),
                                                         1 + rng() % (g_max_threads < 12 ? g_max_threads : 12), rcs.data(), H263MI_STRENGTH_FROM_HEADER, (uint8_t *const *)bufs.data(),
                                                         caps.data(), nullptr);
        CHECK(rc == H263MI_OK);
        for (uint32_t s = 0; s < n; s++)
            if (data[s]) {
                CHECK(rcs[s] == H263MI_OK);
                if (rcs[s] == H263MI_OK) next[s]++;
            }
        if (c % 5 == 4) CHECK(h263mi_mixed_sync(m, nullptr) == H263MI_OK);
    }
    CHECK(h263mi_mixed_sync(m, nullptr) == H263MI_OK);
    h263mi_mixed_destroy(m);
    for (void *p : bufs) CHECK(h263mi_device_free(0, p) == H263MI_OK);
}

// One call of a mixed-size set: pick[s] = {corpus (0: no picture, 1: the first, 2: the second), frame}.  rcs / used: per stream.
struct MixedCall {
    h263mi_mixed *m = nullptr;
    std::vector<void *> bufs;
    std::vector<size_t> caps;
    MixedCall(uint32_t n, bool pipeline)
    {
        h263mi_backend_cfg cfg{0, pipeline ? H263MI_CFG_PIPELINE_POST : 0u, nullptr};
        CHECK(h263mi_mixed_create(n, &cfg, &m) == H263MI_OK);
        bufs.assign(n, nullptr);
        caps.assign(n, (size_t)std::max(g_w * g_h, g_w2 * g_h2) * 4);
        for (uint32_t s = 0; s < n; s++) CHECK(h263mi_device_malloc(0, caps[s], &bufs[s]) == H263MI_OK);
    }
    ~MixedCall()
    {
        h263mi_mixed_destroy(m);
        for (void *p : bufs) CHECK(h263mi_device_free(0, p) == H263MI_OK);
    }
    struct Pick { int corpus; uint32_t frame; };
    int call(const std::vector<Pick> &pick, std::vector<int> &rcs, std::vector<size_t> &used)
    {
        const size_t n = bufs.size();
        std::vector<const uint8_t *> data(n, nullptr);
        std::vector<size_t> len(n, 0);
        rcs.assign(n, -1);
        used.assign(n, 99);
        for (size_t s = 0; s < n && s < pick.size(); s++) {
            if (!pick[s].corpus) continue;
            const auto &c = pick[s].corpus == 1 ? g_corpus : g_corpus2;
            const std::vector<uint8_t> &p = c[s % c.size()][pick[s].frame % c[0].size()];
            data[s] = p.data();
            len[s] = p.size();
        }
        return h263mi_mixed_decode_next_pictures_ps(m, H263MI_SORENSON_SPARK_BITSTREAM, data.data(), len.data(), used.data(), 2, rcs.data(),
                                                    H263MI_STRENGTH_FROM_HEADER, nullptr, (uint8_t *const *)bufs.data(), caps.data(), nullptr);
    }
    // per stream: (rc, width, height) of h263mi_mixed_stream_size
    std::vector<uint64_t> sizes() const
    {
        std::vector<uint64_t> v;
        for (uint32_t s = 0; s < bufs.size(); s++) {
            uint16_t w = 0, h = 0;
            v.push_back((uint64_t)(int64_t)h263mi_mixed_stream_size(m, s, &w, &h));
            v.push_back(w);
            v.push_back(h);
        }
        return v;
    }
};

// A mixed-size set over both corpora: streams move between the two classes at key frames, a P picture of the other size is
// refused and leaves the stream as it was, a class doubles when streams join a full one, and the sync that finds a class at most
// a quarter full shrinks it.  (slots_bytes: a class of k slots holds 2k frames of its size.)
static void drive_mixed_sizes(bool pipeline)
{
    const uint32_t n = 8;
    MixedCall mc(n, pipeline);
    if (!mc.m) return;
    typedef MixedCall::Pick Pick;
    std::vector<int> rcs;
    std::vector<size_t> used;
    std::vector<uint32_t> next(n, 0);
    // every stream in `streams` sends its next picture of `corpus` (frame 0: a key frame); all must decode
    auto step = [&](std::initializer_list<uint32_t> streams, int corpus) {
        std::vector<Pick> pick(n, Pick{0, 0});
        for (uint32_t s : streams) pick[s] = Pick{corpus, next[s]};
        CHECK(mc.call(pick, rcs, used) == H263MI_OK);
        for (uint32_t s : streams) {
            CHECK(rcs[s] == H263MI_OK && used[s] > 0);
            next[s]++;
        }
    };
    auto size_is = [&](uint32_t s, uint16_t w, uint16_t h) {
        uint16_t sw = 0, sh = 0;
        CHECK(h263mi_mixed_stream_size(mc.m, s, &sw, &sh) == H263MI_OK && sw == w && sh == h);
    };
    step({0, 1}, 1);                                             // a class of the first size: 2 slots
    CHECK(h263mi_mixed_size_classes(mc.m) == 1);
    const uint64_t two = h263mi_mixed_frame_store_bytes(mc.m);
    CHECK(two > 0);
    step({2, 3}, 1);                                             // two join a full class: 4 slots
    CHECK(h263mi_mixed_frame_store_bytes(mc.m) == 2 * two);
    step({0, 1, 2, 3, 4, 5, 6, 7}, 1);                           // four more: 8 slots
    CHECK(h263mi_mixed_frame_store_bytes(mc.m) == 4 * two);
    for (uint32_t s = 0; s < n; s++) size_is(s, g_w, g_h);
    // a P picture of the other size: refused, nothing consumed, the stream keeps its size (and its picture)
    {
        std::vector<Pick> pick(n, Pick{0, 0});
        pick[0] = Pick{2, 1};
        pick[1] = Pick{1, next[1]};
        CHECK(mc.call(pick, rcs, used) == H263MI_OK);
        CHECK(rcs[0] == H263MI_ERR_PICTURE_FORMAT_INVALID && used[0] == 0);
        CHECK(rcs[1] == H263MI_OK && used[1] > 0);
        next[1]++;
        size_is(0, g_w, g_h);
    }
    // seven streams move to the second size at a key frame: a class of 8 slots for them; the first class keeps 1 member in 8 slots
    for (uint32_t s = 0; s < n; s++)
        if (s != 1) next[s] = 0;
    step({0, 2, 3, 4, 5, 6, 7}, 2);
    const uint64_t before_shrink = h263mi_mixed_frame_store_bytes(mc.m);
    CHECK(h263mi_mixed_size_classes(mc.m) == 2);
    CHECK(before_shrink > 4 * two);
    size_is(0, g_w2, g_h2);
    size_is(1, g_w, g_h);
    // the sync finds the first class at most a quarter full and shrinks it to 1 slot
    CHECK(h263mi_mixed_sync(mc.m, nullptr) == H263MI_OK);
    CHECK(h263mi_mixed_size_classes(mc.m) == 2);
    CHECK(h263mi_mixed_frame_store_bytes(mc.m) == before_shrink - 4 * two + two / 2);
    for (uint32_t s = 0; s < n; s++) size_is(s, s == 1 ? g_w : g_w2, s == 1 ? g_h : g_h2);
    // P pictures on both classes after the moves, then one stream back to the first size (its class grows to 2 slots)
    step({1}, 1);
    step({0, 2, 3, 4, 5, 6, 7}, 2);
    const uint64_t before_grow = h263mi_mixed_frame_store_bytes(mc.m);
    next[2] = 0;
    step({2}, 1);
    CHECK(h263mi_mixed_frame_store_bytes(mc.m) == before_grow + two / 2);
    size_is(2, g_w, g_h);
    step({1, 2}, 1);
    step({0, 3, 4, 5, 6, 7}, 2);
    CHECK(h263mi_mixed_sync(mc.m, nullptr) == H263MI_OK);
}

// one H263State fed coded pictures (h263mi_decode_next_picture: parse into the state's own staging slot), with the accessors
// and the rendering a consumer calls behind it
static void drive_state(unsigned seed, int pictures)
{
    std::mt19937 rng(seed);
    h263mi_state *st = nullptr;
    CHECK(h263mi_state_new(H263MI_SORENSON_SPARK_BITSTREAM, nullptr, &st) == H263MI_OK);
    if (!st) return;
    std::vector<uint8_t> rgba((size_t)g_w * g_h * 4), y((size_t)g_w * g_h), cb((size_t)g_w * g_h / 4 + 64), cr(cb.size());
    const std::vector<std::vector<uint8_t>> &stream = g_corpus[seed % g_corpus.size()];
    for (int k = 0; k < pictures; k++) {
        const std::vector<uint8_t> &p = stream[(size_t)k % stream.size()];
        size_t used = 0;
        CHECK(h263mi_decode_next_picture(st, p.data(), p.size(), &used) == H263MI_OK);
        h263mi_frame_view v;
        CHECK(h263mi_get_last_picture(st, &v) == H263MI_OK && v.width == g_w && v.height == g_h);
        if (rng() % 2) CHECK(h263mi_render_rgba(st, H263MI_STRENGTH_FROM_HEADER, rgba.data()) == H263MI_OK);
        if (rng() % 4 == 0) CHECK(h263mi_copy_yuv(st, y.data(), cb.data(), cr.data()) == H263MI_OK);
        if (rng() % 16 == 0) CHECK(h263mi_state_reset(st) == H263MI_OK && (k = (k / (int)stream.size() + 1) * (int)stream.size() - 1, true));
    }
    // a truncated picture is that call's error and leaves the state as it was
    const std::vector<uint8_t> &p0 = stream[0];
    size_t used = 0;
    CHECK(h263mi_decode_next_picture(st, p0.data(), 3, &used) != H263MI_OK);
    h263mi_state_free(st);
}

// the entries over DEVICE records (h263mi_batch_decode / _decode_events): the host side of "checked by default" -- sizes not
// given are taken from the allocations (here: the stub's registry of malloc'd blocks), arrays that cannot hold the batch are
// refused before anything is queued, H263MI_STRENGTH_FROM_HEADER has no meaning without a header
static void drive_device_arrays()
{
    const uint32_t n = 3;
    h263mi_backend_cfg cfg{0, H263MI_CFG_PIPELINE_POST, nullptr};
    h263mi_batch *b = nullptr;
    CHECK(h263mi_batch_create(n, g_w, g_h, &cfg, &b) == H263MI_OK);
    if (!b) return;
    const uint32_t per = h263mi_batch_mbs_per_picture(b);
    std::vector<h263mi_mb_record> mbs((size_t)n * per);
    std::vector<int16_t> co((size_t)n * per * 6 * 64);
    std::vector<uint64_t> base(n);
    size_t at = 0;
    for (uint32_t s = 0; s < n; s++) {
        size_t nb = 0;
        base[s] = at;
        CHECK(h263mi_synth_picture_host(H263MI_SYNTH_I_MIXED, g_w, g_h, s, 0, mbs.data() + (size_t)s * per, co.data() + at * 64,
                                        (size_t)per * 6, &nb) == H263MI_OK);
        at += nb;
    }
    void *d_m = nullptr, *d_c = nullptr, *d_b = nullptr, *d_rgba = nullptr, *d_short = nullptr;
    CHECK(h263mi_device_malloc(0, mbs.size() * sizeof mbs[0], &d_m) == H263MI_OK);
    CHECK(h263mi_device_malloc(0, at * 128, &d_c) == H263MI_OK);
    CHECK(h263mi_device_malloc(0, n * 8, &d_b) == H263MI_OK);
    CHECK(h263mi_device_malloc(0, (size_t)n * g_w * g_h * 4, &d_rgba) == H263MI_OK);
    CHECK(h263mi_device_malloc(0, mbs.size() * sizeof mbs[0] - 32, &d_short) == H263MI_OK);
    CHECK(h263mi_device_memcpy_h2d(0, d_m, mbs.data(), mbs.size() * sizeof mbs[0]) == H263MI_OK);
    CHECK(h263mi_device_memcpy_h2d(0, d_c, co.data(), at * 128) == H263MI_OK);
    CHECK(h263mi_device_memcpy_h2d(0, d_b, base.data(), n * 8) == H263MI_OK);
    const uint8_t strengths[3] = {0, 7, 12};
    // no size given: the pool ends where its allocation ends
    CHECK(h263mi_batch_decode_ps(b, H263MI_PICTURE_I, (const h263mi_mb_record *)d_m, (const int16_t *)d_c, (const uint64_t *)d_b, 0, 0,
                                 strengths, (uint8_t *)d_rgba, nullptr) == H263MI_OK);
    CHECK(h263mi_batch_sync(b) == H263MI_OK);
    // a size beyond the allocation, records one short, an output buffer too small, a strength out of range, no header to take it from
    CHECK(h263mi_batch_decode(b, H263MI_PICTURE_I, (const h263mi_mb_record *)d_m, (const int16_t *)d_c, (const uint64_t *)d_b, at + 1, 3,
                              (uint8_t *)d_rgba, nullptr) == H263MI_ERR_INVALID_ARGUMENT);
    CHECK(h263mi_batch_decode(b, H263MI_PICTURE_I, (const h263mi_mb_record *)d_short, (const int16_t *)d_c, (const uint64_t *)d_b, at, 3,
                              (uint8_t *)d_rgba, nullptr) == H263MI_ERR_INVALID_ARGUMENT);
    CHECK(h263mi_batch_decode(b, H263MI_PICTURE_I, (const h263mi_mb_record *)d_m, (const int16_t *)d_c, (const uint64_t *)d_b, at, 3,
                              (uint8_t *)d_b, nullptr) == H263MI_ERR_INVALID_ARGUMENT);
    CHECK(h263mi_batch_decode(b, H263MI_PICTURE_I, (const h263mi_mb_record *)d_m, (const int16_t *)d_c, (const uint64_t *)d_b, at, 13,
                              (uint8_t *)d_rgba, nullptr) == H263MI_ERR_INVALID_ARGUMENT);
    CHECK(h263mi_batch_decode(b, H263MI_PICTURE_I, (const h263mi_mb_record *)d_m, (const int16_t *)d_c, (const uint64_t *)d_b, at,
                              H263MI_STRENGTH_FROM_HEADER, (uint8_t *)d_rgba, nullptr) == H263MI_ERR_INVALID_ARGUMENT);
    // a pointer the runtime does not know (host memory) with no size: refused; on a trusted batch: the caller vouches
    CHECK(h263mi_batch_submit(b, H263MI_PICTURE_I, mbs.data(), co.data(), nullptr) == H263MI_ERR_INVALID_ARGUMENT);
    h263mi_batch_destroy(b);
    cfg.flags |= H263MI_CFG_TRUSTED_ARRAYS;
    CHECK(h263mi_batch_create(n, g_w, g_h, &cfg, &b) == H263MI_OK);
    if (b) {
        CHECK(h263mi_batch_decode(b, H263MI_PICTURE_I, (const h263mi_mb_record *)d_short, (const int16_t *)d_c, (const uint64_t *)d_b, 0, 3,
                                  (uint8_t *)d_rgba, nullptr) == H263MI_OK);       // (stub kernels read nothing of it)
        CHECK(h263mi_batch_sync(b) == H263MI_OK);
        h263mi_batch_destroy(b);
    }
    for (void *p : {d_m, d_c, d_b, d_rgba, d_short}) CHECK(h263mi_device_free(0, p) == H263MI_OK);
}

// the entries over HOST arrays of a caller (h263mi_submit_picture[_events], h263mi_batch_submit_host[_events]) fed GARBAGE: every
// record field, block index, block offset and event word random, in exact-size heap arrays (AddressSanitizer sees one element
// beyond them).  The host validates these before anything is staged: the answer is a refusal or -- garbage that happens to be a
// valid picture -- a decode; never a read outside the arrays, never a changed state behind a refusal.
static void drive_host_garbage(unsigned seed, int tries)
{
    std::mt19937 rng(seed);
    h263mi_state *st = nullptr;
    CHECK(h263mi_state_new(H263MI_SORENSON_SPARK_BITSTREAM, nullptr, &st) == H263MI_OK);
    h263mi_backend_cfg cfg{0, 0, nullptr};
    h263mi_batch *b = nullptr;
    CHECK(h263mi_batch_create(2, g_w, g_h, &cfg, &b) == H263MI_OK);
    if (!st || !b) return;
    const uint32_t per = h263mi_batch_mbs_per_picture(b);
    // a valid key picture first: garbage P pictures then have a reference to be refused against, or to predict from
    std::vector<h263mi_mb_record> key(per);
    std::vector<int16_t> key_co((size_t)per * 6 * 64);
    size_t key_blocks = 0;
    CHECK(h263mi_synth_picture_host(H263MI_SYNTH_I_MIXED, g_w, g_h, 0, 0, key.data(), key_co.data(), (size_t)per * 6, &key_blocks) == H263MI_OK);
    h263mi_picture_desc desc{};
    desc.width = g_w;
    desc.height = g_h;
    desc.picture_type = H263MI_PICTURE_I;
    desc.pquant = 8;
    CHECK(h263mi_submit_picture(st, &desc, key.data(), per, key_co.data(), key_blocks) == H263MI_OK);
    auto acceptable = [](int rc) {
        return rc == H263MI_OK || rc == H263MI_ERR_INVALID_ARGUMENT || rc == H263MI_ERR_UNCODED_IFRAME_BLOCKS ||
               rc == H263MI_ERR_PICTURE_FORMAT_INVALID;
    };
    int refused = 0, taken = 0;
    for (int t = 0; t < tries; t++) {
        const int flavour = (int)(rng() % 4);      // 0: all random; 1: plausible fields, random structure; 2, 3: a valid picture
                                                   // with (2) or without (3) a few wild fields
        const size_t n_mbs = rng() % 3 == 0 ? per : rng() % (per + 1);
        const size_t n_blocks = rng() % 40;
        // exact-size arrays (new[]: a redzone right behind the last element)
        std::unique_ptr<uint32_t[]> first(new uint32_t[n_blocks + 1]);
        uint32_t at = 0;
        for (size_t k = 0; k <= n_blocks; k++) {
            first[k] = flavour ? at : rng();
            at += (uint32_t)(rng() % 9);
        }
        const size_t n_events = flavour >= 2 ? first[n_blocks] : rng() % 200;
        if (flavour == 1 && rng() % 2) first[n_blocks] = (uint32_t)n_events;
        std::unique_ptr<h263mi_mb_record[]> mbs(new h263mi_mb_record[n_mbs ? n_mbs : 1]);
        std::unique_ptr<int16_t[]> co(new int16_t[(n_blocks ? n_blocks : 1) * 64]);
        std::unique_ptr<uint32_t[]> ev(new uint32_t[n_events ? n_events : 1]);
        const uint32_t wild = flavour == 3 ? 0u : (uint32_t)(flavour == 2 ? 2 * per : 50);       // (a wild value in one field of `wild`)
        for (size_t i = 0; i < n_mbs; i++) {
            h263mi_mb_record &m = mbs[i];
            uint32_t *w = reinterpret_cast<uint32_t *>(&m);
            for (size_t k = 0; k < sizeof m / 4; k++) w[k] = rng();
            if (flavour) {
                m.mb_type = (uint8_t)(rng() % 6);
                m.quant = (uint8_t)(1 + rng() % 31);
                m.cbp &= 0x3f;
                m.kill &= 0x3f;
                m.coeff_index = n_blocks ? (uint32_t)(rng() % n_blocks) : 0;
                if (flavour >= 2) {
                    if (n_blocks < 6) m.cbp = 0;
                    else m.coeff_index = (uint32_t)(rng() % (n_blocks - 5));
                }
                if (wild && rng() % wild == 0) m.coeff_index = rng() % 2 ? 0xffffffffu : (uint32_t)n_blocks;
                if (wild && rng() % wild == 0) m.quant = (uint8_t)(rng() % 2 ? 0 : 32);
                if (wild && rng() % wild == 0) m.mb_type = (uint8_t)(6 + rng() % 250);
                if (wild && rng() % wild == 0) m.cbp |= 0x40;
            }
        }
        for (size_t k = 0; k < (n_blocks ? n_blocks : 1) * 64; k++) co[k] = (int16_t)rng();
        for (size_t k = 0; k < n_events; k++) ev[k] = rng();
        if (flavour >= 2)                                  // a block's events name distinct positions
            for (size_t k = 0; k < n_blocks; k++)
                for (uint32_t e = first[k]; e < first[k + 1]; e++) ev[e] = (ev[e] & 0xffff0000u) | ((first[k] + 7u * (e - first[k])) & 63u);
        if (flavour == 2 && n_blocks && rng() % 3 == 0) first[rng() % (n_blocks + 1)] = rng() % 2 ? 0xffffffffu : (uint32_t)n_events + 1;
        if (flavour == 2 && n_events && rng() % 3 == 0) ev[rng() % n_events] = ev[0];
        desc.picture_type = (uint8_t)(flavour >= 2 ? rng() % 2 : rng() % 12);
        if (flavour < 3 && rng() % 20 == 0) desc.width = (uint16_t)rng();
        else desc.width = g_w;
        h263mi_frame_view before{}, after{};
        const int had = h263mi_get_last_picture(st, &before);
        int rc = rng() % 2 ? h263mi_submit_picture(st, &desc, mbs.get(), n_mbs, co.get(), n_blocks)
                           : h263mi_submit_picture_events(st, &desc, mbs.get(), n_mbs, first.get(), n_blocks, ev.get(), n_events);
        CHECK(acceptable(rc));
        if (rc != H263MI_OK) {
            refused++;
            // state.rs:142: on error the state is unchanged
            CHECK(h263mi_get_last_picture(st, &after) == had && (had != H263MI_OK || (after.width == before.width && after.dev_y == before.dev_y && after.temporal_reference == before.temporal_reference)));
        } else {
            taken++;
        }
        // the batch forms: stream 0 the garbage, stream 1 the key picture (or nothing)
        const h263mi_mb_record *bm[2] = {mbs.get(), key.data()};
        const uint32_t bn[2] = {(uint32_t)n_mbs, per};
        const int16_t *bc[2] = {co.get(), key_co.data()};
        const uint32_t bb[2] = {(uint32_t)n_blocks, (uint32_t)key_blocks};
        rc = h263mi_batch_submit_host(b, H263MI_PICTURE_I, bm, bn, bc, bb);
        CHECK(acceptable(rc));
        const uint32_t *bf[2] = {first.get(), nullptr};
        const uint32_t *be[2] = {ev.get(), nullptr};
        const uint32_t bn0[2] = {(uint32_t)n_mbs, 0}, bb0[2] = {(uint32_t)n_blocks, 0}, bne[2] = {(uint32_t)n_events, 0};
        const h263mi_mb_record *bm0[2] = {mbs.get(), nullptr};
        rc = h263mi_batch_submit_host_events(b, H263MI_PICTURE_I, bm0, bn0, bf, bb0, be, bne);
        CHECK(acceptable(rc));
        (void)h263mi_batch_sync(b);
    }
    CHECK(refused > 0);
    fprintf(stderr, "  host garbage: %d refused, %d decoded\n", refused, taken);
    h263mi_batch_destroy(b);
    h263mi_state_free(st);
}

// a synthetic picture in both host forms: dense blocks and events (level << 16 | position)
struct HostPicture {
    h263mi_picture_desc desc{};
    std::vector<h263mi_mb_record> mbs;
    std::vector<int16_t> co;
    std::vector<uint32_t> first, ev;
    size_t blocks = 0;
};
static HostPicture host_picture(int kind, uint16_t w, uint16_t h, uint32_t seed, uint16_t temporal_reference)
{
    HostPicture p;
    const size_t per = (size_t)((w + 15) / 16) * ((h + 15) / 16);
    p.mbs.resize(per);
    p.co.resize(per * 6 * 64);
    CHECK(h263mi_synth_picture_host(kind, w, h, seed, 0, p.mbs.data(), p.co.data(), per * 6, &p.blocks) == H263MI_OK);
    p.first.push_back(0);
    for (size_t k = 0; k < p.blocks; k++) {
        for (uint32_t pos = 0; pos < 64; pos++)
            if (p.co[k * 64 + pos]) p.ev.push_back((uint32_t)(uint16_t)p.co[k * 64 + pos] << 16 | pos);
        p.first.push_back((uint32_t)p.ev.size());
    }
    p.desc.width = w;
    p.desc.height = h;
    p.desc.picture_type = kind == H263MI_SYNTH_P ? H263MI_PICTURE_P : H263MI_PICTURE_I;
    p.desc.pquant = 8;
    p.desc.temporal_reference = temporal_reference;
    return p;
}
static int submit_dense(h263mi_state *st, const HostPicture &p)
{
    return h263mi_submit_picture(st, &p.desc, p.mbs.data(), p.mbs.size(), p.co.data(), p.blocks);
}
static int submit_events(h263mi_state *st, const HostPicture &p)
{
    return h263mi_submit_picture_events(st, &p.desc, p.mbs.data(), p.mbs.size(), p.first.data(), p.blocks, p.ev.data(), p.ev.size());
}
// what a refused call must leave as it was: the last picture's size, planes and temporal reference
static std::vector<uint64_t> last_picture(const h263mi_state *st)
{
    h263mi_frame_view v{};
    const int rc = h263mi_get_last_picture(st, &v);
    return {(uint64_t)(int64_t)rc, v.width, v.height, (uint64_t)(uintptr_t)v.dev_y, v.temporal_reference};
}

// h263mi_debug_fail_nth_hip_call at every HIP call of one call, each time on objects made afresh: the call reports the failure and
// changes nothing that can be seen, and the same call then goes through (nothing was left half-made).  may_absorb: a failure the
// call may get over by itself (h263mi_decode_next_picture parses into the staging slot only when that slot is to be had).
struct SweepSubject {
    virtual ~SweepSubject() {}
    virtual int call() = 0;
    virtual std::vector<uint64_t> view() = 0;
};
static void fault_sweep(const char *name, bool may_absorb, const std::function<SweepSubject *()> &make, int min_failures = 3)
{
    int failures = 0;
    for (int nth = 1; nth < 500; nth++) {
        std::unique_ptr<SweepSubject> s(make());
        const std::vector<uint64_t> before = s->view();
        h263mi_debug_fail_nth_hip_call(nth);
        const int rc = s->call();
        const bool fired = h263mi_debug_fail_nth_hip_call(0) <= 0;
        if (rc == H263MI_OK && !fired) {
            fprintf(stderr, "  fault sweep %s: %d failures\n", name, failures);
            CHECK(failures >= min_failures);
            return;
        }
        if (rc == H263MI_OK) {
            CHECK(may_absorb);
            continue;
        }
        failures++;
        CHECK(fired && rc == H263MI_ERR_OUT_OF_MEMORY);
        CHECK(s->view() == before);
        CHECK(s->call() == H263MI_OK);
    }
    CHECK(!"the call never went through");
}

// h263mi_debug_fail_nth_hip_call at every HIP call of a mixed-size set's call, each time on a set made afresh: 3 streams, two of
// the first size and one of the second; in the swept call stream 1 moves to the second size (that class grows).  A failed class
// launch is reported in stream_rc and the call itself may return OK; a failed rendering is the call's error after the pictures
// were decoded.  So what holds at every point is what tests/test_gpu_round5.py checks on the device: a stream reports OK exactly
// when it consumed its picture, a stream with an error keeps its size and picture, a failure is reported somewhere, and a clean
// call afterwards goes through and leaves the classes as large as a run without the failure does.
static void mixed_fault_sweep(bool pipeline)
{
    typedef MixedCall::Pick Pick;
    const std::vector<Pick> keys = {{1, 0}, {1, 0}, {2, 0}}, swept = {{1, 1}, {2, 0}, {2, 1}};
    uint64_t clean_bytes = 0;                    // the frame stores after the two calls without a failure
    {
        MixedCall mc(3, pipeline);
        std::vector<int> rcs;
        std::vector<size_t> used;
        CHECK(mc.call(keys, rcs, used) == H263MI_OK && mc.call(swept, rcs, used) == H263MI_OK);
        CHECK(h263mi_mixed_sync(mc.m, nullptr) == H263MI_OK);
        clean_bytes = h263mi_mixed_frame_store_bytes(mc.m);
    }
    int failures = 0;
    for (int nth = 1; nth < 500; nth++) {
        MixedCall mc(3, pipeline);
        if (!mc.m) return;
        std::vector<int> rcs;
        std::vector<size_t> used;
        CHECK(mc.call(keys, rcs, used) == H263MI_OK && rcs == std::vector<int>(3, H263MI_OK));
        CHECK(h263mi_mixed_sync(mc.m, nullptr) == H263MI_OK);
        const std::vector<uint64_t> before = mc.sizes();
        h263mi_debug_fail_nth_hip_call(nth);
        const int rc = mc.call(swept, rcs, used);
        const bool fired = h263mi_debug_fail_nth_hip_call(0) <= 0;
        const std::vector<uint64_t> after = mc.sizes();
        bool any_rc = false;
        for (size_t s = 0; s < 3; s++) {
            CHECK((rcs[s] == H263MI_OK) == (used[s] > 0));
            if (rcs[s] != H263MI_OK) {
                any_rc = true;
                CHECK(std::equal(after.begin() + 3 * s, after.begin() + 3 * s + 3, before.begin() + 3 * s));
            }
        }
        if (!fired) {
            CHECK(rc == H263MI_OK && !any_rc);
            fprintf(stderr, "  fault sweep h263mi_mixed_decode_next_pictures_ps (pipeline %d): %d failures\n", (int)pipeline, failures);
            CHECK(failures >= 8);
            return;
        }
        failures++;
        CHECK(rc != H263MI_OK || any_rc);
        // the same pictures once more, without a failure: every stream decodes (the ones that advanced predict from them again),
        // and the classes hold what they would have without the failure (a joiner whose launch failed gave its new slot back)
        CHECK(mc.call(swept, rcs, used) == H263MI_OK && rcs == std::vector<int>(3, H263MI_OK));
        CHECK(h263mi_mixed_sync(mc.m, nullptr) == H263MI_OK);
        CHECK(h263mi_mixed_frame_store_bytes(mc.m) == clean_bytes);
    }
    CHECK(!"the mixed-size call never went through");
}

static void drive_fault_sweeps()
{
    const long live0 = stub_live_allocations();
    static HostPicture key, key2, p, p_short;
    key = host_picture(H263MI_SYNTH_I_MIXED, g_w, g_h, 1, 7);
    key2 = host_picture(H263MI_SYNTH_I_MIXED, 128, 96, 2, 9);
    p = host_picture(H263MI_SYNTH_P, g_w, g_h, 3, 8);
    p_short = p;
    p_short.mbs.pop_back();                           // (the last macroblock is padded as Inter)
    struct State : SweepSubject {
        h263mi_state *st = nullptr;
        std::function<int(h263mi_state *)> fn;
        State(std::function<int(h263mi_state *)> f, bool from_bitstream) : fn(f)
        {
            CHECK(h263mi_state_new(H263MI_SORENSON_SPARK_BITSTREAM, nullptr, &st) == H263MI_OK);
            if (from_bitstream) CHECK(h263mi_decode_next_picture(st, g_corpus[0][0].data(), g_corpus[0][0].size(), nullptr) == H263MI_OK);
            else CHECK(submit_dense(st, key) == H263MI_OK);
        }
        ~State() { h263mi_state_free(st); }
        int call() override { return fn(st); }
        std::vector<uint64_t> view() override { return last_picture(st); }
    };
    fault_sweep("h263mi_submit_picture", false, [] { return new State([](h263mi_state *st) { return submit_dense(st, p); }, false); });
    fault_sweep("h263mi_submit_picture (size change)", false,
                [] { return new State([](h263mi_state *st) { return submit_dense(st, key2); }, false); });
    fault_sweep("h263mi_submit_picture_events", false,
                [] { return new State([](h263mi_state *st) { return submit_events(st, p_short); }, false); });
    fault_sweep("h263mi_decode_next_picture", true, [] {
        return new State([](h263mi_state *st) {
            const std::vector<uint8_t> &pic = g_corpus[0][1];
            return h263mi_decode_next_picture(st, pic.data(), pic.size(), nullptr);
        }, true);
    });
    struct Batch : SweepSubject {
        h263mi_batch *b = nullptr;
        Batch()
        {
            h263mi_backend_cfg cfg{0, 0, nullptr};
            CHECK(h263mi_batch_create(2, g_w, g_h, &cfg, &b) == H263MI_OK);
            const h263mi_mb_record *m[2] = {key.mbs.data(), key.mbs.data()};
            const int16_t *c[2] = {key.co.data(), key.co.data()};
            const uint32_t n[2] = {(uint32_t)key.mbs.size(), (uint32_t)key.mbs.size()}, nb[2] = {(uint32_t)key.blocks, (uint32_t)key.blocks};
            CHECK(h263mi_batch_submit_host(b, H263MI_PICTURE_I, m, n, c, nb) == H263MI_OK);
            CHECK(h263mi_batch_sync(b) == H263MI_OK);
        }
        ~Batch() { h263mi_batch_destroy(b); }
        int call() override
        {
            const h263mi_mb_record *m[2] = {p.mbs.data(), p_short.mbs.data()};
            const int16_t *c[2] = {p.co.data(), p.co.data()};
            const uint32_t n[2] = {(uint32_t)p.mbs.size(), (uint32_t)p_short.mbs.size()}, nb[2] = {(uint32_t)p.blocks, (uint32_t)p.blocks};
            return h263mi_batch_submit_host(b, H263MI_PICTURE_P, m, n, c, nb);
        }
        std::vector<uint64_t> view() override
        {
            return {(uint64_t)h263mi_batch_stream_has_picture(b, 0), (uint64_t)h263mi_batch_stream_has_picture(b, 1)};
        }
    };
    fault_sweep("h263mi_batch_submit_host (2 streams)", false, [] { return new Batch(); });
    // the bitstream entry of a batch: 2 streams, P pictures behind their key frames, rendered with the headers' strengths
    struct BatchBitstream : SweepSubject {
        h263mi_batch *b = nullptr;
        void *d_rgba = nullptr;
        BatchBitstream()
        {
            h263mi_backend_cfg cfg{0, 0, nullptr};
            CHECK(h263mi_batch_create(2, g_w, g_h, &cfg, &b) == H263MI_OK);
            CHECK(h263mi_device_malloc(0, (size_t)2 * g_w * g_h * 4, &d_rgba) == H263MI_OK);
            CHECK(decode(0) == H263MI_OK);
            CHECK(h263mi_batch_sync(b) == H263MI_OK);
        }
        ~BatchBitstream()
        {
            h263mi_batch_destroy(b);
            CHECK(h263mi_device_free(0, d_rgba) == H263MI_OK);
        }
        int decode(uint32_t frame)
        {
            const uint8_t *data[2] = {g_corpus[0][frame].data(), g_corpus[1][frame].data()};
            const size_t len[2] = {g_corpus[0][frame].size(), g_corpus[1][frame].size()};
            size_t used[2] = {0, 0};
            int rcs[2] = {-1, -1};
            return h263mi_batch_decode_next_pictures_ps(b, H263MI_SORENSON_SPARK_BITSTREAM, data, len, used, 2, rcs,
                                                        H263MI_STRENGTH_FROM_HEADER, nullptr, (uint8_t *)d_rgba, nullptr);
        }
        int call() override { return decode(1); }
        std::vector<uint64_t> view() override
        {
            return {(uint64_t)h263mi_batch_stream_has_picture(b, 0), (uint64_t)h263mi_batch_stream_has_picture(b, 1)};
        }
    };
    fault_sweep("h263mi_batch_decode_next_pictures_ps (2 streams)", false, [] { return new BatchBitstream(); });
    // the shaped renderings of a state: each makes a shape (device offsets, or a scratch and span tables) and grows the state's
    // own scratch on the way
    static std::vector<uint8_t> host_out((size_t)1 << 18);
    fault_sweep("h263mi_render_rgba_layout", false, [] {
        return new State([](h263mi_state *st) {
            h263mi_rgba_layout l{};
            l.scale_log2 = 1;
            l.row_pitch = 512;
            return h263mi_render_rgba_layout(st, 5, &l, host_out.data());
        }, false);
    });
    fault_sweep("h263mi_render_rgba_resize", false, [] {
        return new State([](h263mi_state *st) {
            h263mi_rgba_resize r{};
            r.out_width = 100, r.out_height = 60, r.row_pitch = 512;
            return h263mi_render_rgba_resize(st, 5, &r, host_out.data());
        }, false);
    });
    fault_sweep("h263mi_render_yuv", false, [] {
        return new State([](h263mi_state *st) {
            h263mi_yuv_layout l{};
            l.format = H263MI_YUV_NV12;
            l.pitch_y = l.pitch_c = 200;
            return h263mi_render_yuv(st, 5, &l, host_out.data());
        }, false);
    });
    fault_sweep("h263mi_render_yuv_resize", false, [] {
        return new State([](h263mi_state *st) {
            h263mi_yuv_resize r{};
            r.out_width = 100, r.out_height = 60, r.format = H263MI_YUV_I420;
            return h263mi_render_yuv_resize(st, 5, &r, host_out.data());
        }, false);
    });
    // the setters of a batch's output shape, each over a batch that has another shape of that kind in force: a setter that fails
    // leaves it in force -- one rendering (RGBA and planes) launches what it launched before
    struct BatchShape : Batch {
        void *d_out = nullptr;
        std::function<int(h263mi_batch *)> setter;
        explicit BatchShape(std::function<int(h263mi_batch *)> f) : setter(f)
        {
            CHECK(h263mi_device_malloc(0, (size_t)1 << 20, &d_out) == H263MI_OK);
            stub_trace_output(d_out);
            h263mi_rgba_layout l{};
            l.scale_log2 = 1;
            l.row_pitch = 512;
            CHECK(h263mi_batch_set_rgba_layout(b, &l) == H263MI_OK);
            h263mi_yuv_layout y{};
            y.format = H263MI_YUV_NV12;
            y.pitch_y = y.pitch_c = 256;
            CHECK(h263mi_batch_set_yuv_layout(b, &y) == H263MI_OK);
        }
        ~BatchShape() { CHECK(h263mi_device_free(0, d_out) == H263MI_OK); }
        int call() override { return setter(b); }
        std::vector<uint64_t> view() override
        {
            std::string trace;
            stub_trace_into(&trace);
            CHECK(h263mi_batch_render_rgba_ps(b, 5, nullptr, (uint8_t *)d_out, (uint8_t *)d_out + ((size_t)1 << 19)) == H263MI_OK);
            stub_trace_into(nullptr);
            // what the rendering launched, without what moves on from one rendering to the next: the event lines and the slot of
            // an upload ring that an array lies in ("@lib:<bytes>+<offset>[")
            std::vector<uint64_t> v;
            for (size_t at = 0; at < trace.size();) {
                const size_t end = trace.find('\n', at);
                const std::string line = trace.substr(at, end - at);
                at = end + 1;
                if (line.compare(0, 7, "record ") == 0 || line.compare(0, 5, "wait ") == 0) continue;
                for (size_t k = 0; k < line.size(); k++) {
                    if (line[k] == '@') k = line.find('[', k);
                    v.push_back((uint8_t)line[k]);
                }
                v.push_back('\n');
            }
            CHECK(v.size() > 100);
            return v;
        }
    };
    fault_sweep("h263mi_batch_set_rgba_resize", false, [] {
        return new BatchShape([](h263mi_batch *b) {
            h263mi_rgba_resize r{};
            r.out_width = 100, r.out_height = 60;
            return h263mi_batch_set_rgba_resize(b, &r);
        });
    });
    fault_sweep("h263mi_batch_set_yuv_layout", false, [] {
        return new BatchShape([](h263mi_batch *b) {
            h263mi_yuv_layout l{};
            l.format = H263MI_YUV_I420;
            l.pitch_y = 200, l.pitch_c = 100;
            return h263mi_batch_set_yuv_layout(b, &l);
        });
    }, /*min_failures=*/2);              // (an allocation and a copy)
    fault_sweep("h263mi_batch_set_yuv_resize", false, [] {
        return new BatchShape([](h263mi_batch *b) {
            h263mi_yuv_resize r{};
            r.out_width = 100, r.out_height = 60, r.format = H263MI_YUV_NV12;
            return h263mi_batch_set_yuv_resize(b, &r);
        });
    });
    if (!g_corpus2.empty())
        for (bool pipeline : {false, true}) mixed_fault_sweep(pipeline);
    // every pinned and device block and every event of the objects above went with them
    CHECK(stub_live_allocations() == live0);
    CHECK(live0 == 0);
}

// The order in which h263mi_submit_picture[_events] names what is wrong with a call.  Every case breaks one rule and, where it
// can, a later one with another code as well: a reordering of the checks changes the answer.
static void drive_state_precedence()
{
    const HostPicture key = host_picture(H263MI_SYNTH_I_MIXED, g_w, g_h, 11, 1);
    const HostPicture p = host_picture(H263MI_SYNTH_P, g_w, g_h, 12, 2);
    const HostPicture p2 = host_picture(H263MI_SYNTH_P, 128, 96, 13, 3);
    const size_t total = p.mbs.size();
    enum Start { kFresh, kKeyed, kKeyedThenReset };
    struct Case {
        const char *name;
        Start start;
        int want;
        std::function<int(h263mi_state *)> call;
    };
    auto no_size = [](HostPicture q) { q.desc.width = 0; return q; };
    size_t dup_block = 0;                                // a block with two events or more
    while (dup_block < p.blocks && p.first[dup_block + 1] - p.first[dup_block] < 2) dup_block++;
    CHECK(dup_block < p.blocks);
    size_t coded = 0;                                    // a record with coded blocks
    while (coded < total && !p.mbs[coded].cbp) coded++;
    CHECK(coded < total);
    const int INV = H263MI_ERR_INVALID_ARGUMENT, PFI = H263MI_ERR_PICTURE_FORMAT_INVALID, UIB = H263MI_ERR_UNCODED_IFRAME_BLOCKS;
    const std::vector<Case> cases = {
        {"valid P, dense", kKeyed, H263MI_OK, [&](h263mi_state *st) { return submit_dense(st, p); }},
        {"valid P, events", kKeyed, H263MI_OK, [&](h263mi_state *st) { return submit_events(st, p); }},
        // 1. the _events entry: no block offsets, too many blocks
        {"1 no block_first_event", kKeyed, INV, [&](h263mi_state *st) {
             const HostPicture q = no_size(p);
             return h263mi_submit_picture_events(st, &q.desc, q.mbs.data(), total, nullptr, q.blocks, q.ev.data(), q.ev.size());
         }},
        {"1 n_coeff_blocks > 2^32/8", kKeyed, INV, [&](h263mi_state *st) {
             const HostPicture q = no_size(p);
             return h263mi_submit_picture_events(st, &q.desc, q.mbs.data(), total, q.first.data(), 0xffffffffu / 8u + 1, q.ev.data(), q.ev.size());
         }},
        // 2. null arrays
        {"2 no records", kKeyed, INV, [&](h263mi_state *st) {
             const HostPicture q = no_size(p);
             return h263mi_submit_picture(st, &q.desc, nullptr, total, q.co.data(), q.blocks);
         }},
        {"2 no coefficients", kKeyed, INV, [&](h263mi_state *st) {
             const HostPicture q = no_size(p);
             return h263mi_submit_picture(st, &q.desc, q.mbs.data(), total, nullptr, q.blocks);
         }},
        {"2 no events", kKeyed, INV, [&](h263mi_state *st) {
             const HostPicture q = no_size(p);
             return h263mi_submit_picture_events(st, &q.desc, q.mbs.data(), total, q.first.data(), q.blocks, nullptr, q.ev.size());
         }},
        // 3. the event lists
        {"3 offsets not from 0", kKeyed, INV, [&](h263mi_state *st) {
             HostPicture q = no_size(p);
             q.first[0] = 1;
             return submit_events(st, q);
         }},
        {"3 a position twice", kKeyed, INV, [&](h263mi_state *st) {
             HostPicture q = no_size(p);
             q.ev[q.first[dup_block] + 1] = q.ev[q.first[dup_block]];
             return submit_events(st, q);
         }},
        // 4. the size
        {"4 zero width", kKeyed, PFI, [&](h263mi_state *st) {
             HostPicture q = no_size(p);
             q.desc.picture_type = 99;
             return submit_dense(st, q);
         }},
        {"4 too large", kKeyed, PFI, [&](h263mi_state *st) {
             HostPicture q = p;
             q.desc.width = q.desc.height = 65535;
             q.desc.picture_type = 99;
             return submit_dense(st, q);
         }},
        // 5. the picture type, 6. the record count, 7. the records -- before the reference (8)
        {"5 picture type", kFresh, INV, [&](h263mi_state *st) {
             HostPicture q = p;
             q.desc.picture_type = H263MI_PICTURE_RESERVED + 1;
             return submit_dense(st, q);
         }},
        {"6 more records than macroblocks", kFresh, INV, [&](h263mi_state *st) {
             HostPicture q = p;
             q.mbs.push_back(q.mbs[0]);
             return submit_dense(st, q);
         }},
        {"7 quantiser 0", kFresh, INV, [&](h263mi_state *st) {
             HostPicture q = p;
             q.mbs[total - 1].quant = 0;
             return submit_dense(st, q);
         }},
        {"7 blocks beyond the pool", kFresh, INV, [&](h263mi_state *st) {
             HostPicture q = p;
             q.mbs[coded].coeff_index = (uint32_t)q.blocks;
             return submit_events(st, q);
         }},
        // 8. no reference -- before 9. a size change under prediction
        {"8 inter without a reference", kKeyedThenReset, UIB, [&](h263mi_state *st) { return submit_dense(st, p2); }},
        {"9 inter across a size change", kKeyed, PFI, [&](h263mi_state *st) { return submit_dense(st, p2); }},
        // the caps of the batch's host path, ahead of the event lists: at most 2^25 blocks, kMaxEventWords events
        {"cap blocks", kKeyed, INV, [&](h263mi_state *st) {
             const HostPicture q = no_size(p);
             return h263mi_submit_picture(st, &q.desc, q.mbs.data(), total, q.co.data(), ((size_t)1 << 25) + 1);
         }},
        {"cap events", kKeyed, INV, [&](h263mi_state *st) {
             const HostPicture q = no_size(p);
             return h263mi_submit_picture_events(st, &q.desc, q.mbs.data(), 0, q.first.data(), 0, q.ev.data(), 0xffffff01u);
         }},
        {"cap events, an otherwise valid picture", kKeyed, INV, [&](h263mi_state *st) {
             return h263mi_submit_picture_events(st, &p.desc, p.mbs.data(), 0, p.first.data(), 0, p.ev.data(), 0xffffff01u);
         }},
    };
    for (const Case &c : cases) {
        h263mi_state *st = nullptr;
        CHECK(h263mi_state_new(H263MI_SORENSON_SPARK_BITSTREAM, nullptr, &st) == H263MI_OK);
        if (!st) return;
        if (c.start != kFresh) CHECK(submit_dense(st, key) == H263MI_OK);
        if (c.start == kKeyedThenReset) CHECK(h263mi_state_reset(st) == H263MI_OK);
        const std::vector<uint64_t> before = last_picture(st);
        const int rc = c.call(st);
        fprintf(stderr, "  precedence %-40s %d\n", c.name, rc);
        CHECK(rc == c.want);
        if (rc != H263MI_OK) CHECK(last_picture(st) == before);
        h263mi_state_free(st);
    }
}

int main(int argc, char **argv)
{
    if (argc < 2 || !load_corpus(argv[1], g_corpus, g_w, g_h) || (argc > 4 && !load_corpus(argv[4], g_corpus2, g_w2, g_h2))) {
        fprintf(stderr, "usage: tsan_driver <corpus.bin> [rounds [max threads [corpus of another size.bin]]]\n");
        return 2;
    }
    const int rounds = argc > 2 ? atoi(argv[2]) : 2;
    if (argc > 3) g_max_threads = (uint32_t)atoi(argv[3]);
    const uint32_t n = (uint32_t)g_corpus.size();
    drive_fault_sweeps();
    drive_state_precedence();
    drive_device_arrays();
    drive_host_garbage(900, 400);
    if (!g_corpus2.empty())
        for (bool pipeline : {false, true}) drive_mixed_sizes(pipeline);
    for (int r = 0; r < rounds; r++) {
        // one batch after the other: spinning and parking plans, teardown parked and mid-spin
        drive_batch(100 + r, n, 40, /*pipeline=*/true, /*destroy_mid_spin=*/false);
        drive_batch(200 + r, n, 25, /*pipeline=*/false, /*destroy_mid_spin=*/true);
        drive_batch(300 + r, 3, 30, /*pipeline=*/true, /*destroy_mid_spin=*/true);        // fewer streams than threads
        // distinct objects from distinct threads at the same time
        std::thread t1(drive_batch, 400 + r, n, 30, true, true);
        std::thread t2(drive_batch, 500 + r, n / 2 + 1, 30, false, false);
        std::thread t3(drive_mixed, 600 + r, n, 20);
        std::thread t4(drive_state, 700 + r, 40);
        t1.join();
        t2.join();
        t3.join();
        t4.join();
    }
    const int bad = g_failures.load();
    fprintf(stderr, "tsan_driver: %d rounds, %d check failures\n", rounds, bad);
    return bad ? 1 : 0;
}
