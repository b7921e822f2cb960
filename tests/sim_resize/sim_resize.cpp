// sim_resize.cpp -- CPU logic checker of k_rgba_resize (TEST INFRASTRUCTURE).
//
// Runs resize_item of h263-rs_amd/csrc/resize_kernel.inl lane by lane: every wave of the launch (band, segment, picture), its
// 64 lanes one after the other in each phase, the LDS hand-off a plain struct.  Built by tests/test_sim_rgba_resize.py with
// g++ -fsanitize=address,undefined into a temporary directory; never part of the product.
//
//   sim_resize <in> <out>
//   in : u32 w, h, ow, oh, n_pictures, pitch; u64 canvas_bytes; u64 offsets[n_pictures] (~0 = the picture is skipped);
//        n_pictures full-size pictures, w*h*4 bytes each; canvas_bytes of canvas
//   out: the canvas after the launch
//   sim_resize --div <d>
//        resize_div(n, d) == n / d for n = q*d - 1, q*d, q*d + d/2, q = 0..255; prints the mismatches, exit status 1 if any
#include <stdlib.h>

#include "../../h263-rs_amd/csrc/resize_kernel.inl"
#include "../sim_common.h"

using namespace h263mi;

static int check_div(uint32_t d)
{
    const float inv_d = 1.0f / (float)d;
    int bad = 0;
    for (uint64_t q = 0; q <= 255; q++) {
        const uint64_t ns[3] = {q * d - (q ? 1 : 0), q * d, q * d + d / 2};
        for (uint64_t n : ns) {
            const uint32_t got = resize_div(n, d, inv_d), want = (uint32_t)(n / d);
            if (got != want) {
                if (bad < 10) printf("d=%u n=%llu: %u, want %u\n", d, (unsigned long long)n, got, want);
                bad++;
            }
        }
    }
    return bad ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "--div")) return check_div((uint32_t)strtoull(argv[2], nullptr, 10));
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    uint32_t hd[6];
    uint64_t canvas_bytes = 0;
    if (!read_all(in, hd, sizeof hd) || !read_all(in, &canvas_bytes, 8)) return 2;
    const uint32_t w = hd[0], h = hd[1], ow = hd[2], oh = hd[3], n = hd[4], pitch = hd[5];
    std::vector<uint64_t> offsets(n);
    if (!read_all(in, offsets.data(), 8 * (size_t)n)) return 2;
    // (exactly as large as the data: ASan sees a read or a write one byte outside)
    std::vector<uint8_t> src((size_t)n * w * h * 4), canvas(canvas_bytes);
    if (!read_all(in, src.data(), src.size()) || !read_all(in, canvas.data(), canvas.size())) return 2;
    fclose(in);

    std::vector<uint8_t *> dst(n);
    for (uint32_t p = 0; p < n; p++) dst[p] = offsets[p] == ~0ull ? nullptr : canvas.data() + offsets[p];
    std::vector<ResizeSpan> spans((size_t)ow + oh);
    resize_spans(w, ow, spans.data());
    resize_spans(h, oh, spans.data() + ow);
    ResizeArgs a{};
    a.src = src.data();
    a.dst = dst.data();
    a.cols = spans.data();
    a.rows = spans.data() + ow;
    a.w = w;
    a.h = h;
    a.ow = ow;
    a.oh = oh;
    a.pitch = pitch;
    a.d = w * h;
    a.inv_d = 1.0f / (float)a.d;
    a.n_pictures = n;
    LaunchDims d;
    if (n) {                                             // (as launch_rgba_resize: no picture, no launch)
        if (!resize_plan(a, d)) return 2;
        run_banded<ResizeLds, ResizeLane>(d, a.bands, a.chunk, [&](ResizeLds &lds, uint32_t band, uint32_t z, uint32_t p, auto each) {
            resize_item(a, lds, band, z, p, each);
        });
    }
    return write_canvas(argv[2], canvas);
}
