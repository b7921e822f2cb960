// sim_yuv_resize.cpp -- CPU logic checker of k_plane_resize (TEST INFRASTRUCTURE).
//
// Runs plane_resize_item of h263-rs_amd/csrc/plane_resize_kernel.inl lane by lane: every wave of the launch (band, segment,
// picture), its 64 lanes one after the other in each phase, the LDS hand-off a plain struct.  Built by
// tests/test_sim_yuv_resize.py with g++ -fsanitize=address,undefined into a temporary directory; never part of the product.
//
//   sim_yuv_resize <in> <out>
//   in : u32 w, h, ow, oh, n_pictures, nv12, pitch_y, pitch_c; u64 canvas_bytes; u64 offsets[3 * n_pictures] (Y, Cb or CbCr, Cr;
//        Y = ~0: the picture is skipped); n_pictures tight I420 pictures, w*h + 2*cw*ch bytes each; canvas_bytes of canvas
//   out: the canvas after the launch
//   sim_yuv_resize --div <d>
//        resize_div(n, d) == n / d for n = q*d - 1, q*d, q*d + d/2, q = 0..255 (q = 255 with + d/2 is a constant plane of 255,
//        q = 0 one of 0, at pw*ph = d); prints the mismatches, exit status 1 if any
#include <stdlib.h>

#include "../../h263-rs_amd/csrc/plane_resize_kernel.inl"
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
    uint32_t hd[8];
    uint64_t canvas_bytes = 0;
    if (!read_all(in, hd, sizeof hd) || !read_all(in, &canvas_bytes, 8)) return 2;
    const uint32_t w = hd[0], h = hd[1], ow = hd[2], oh = hd[3], n = hd[4], nv12 = hd[5], pitch_y = hd[6], pitch_c = hd[7];
    const uint32_t cw = (w + 1) / 2, ch = (h + 1) / 2, cow = (ow + 1) / 2, coh = (oh + 1) / 2;
    std::vector<uint64_t> offsets(3 * (size_t)n);
    if (!read_all(in, offsets.data(), 8 * offsets.size())) return 2;
    // (exactly as large as the data: ASan sees a read or a write one byte outside; operator new aligns both to 16 bytes)
    std::vector<uint8_t> src((size_t)n * (w * h + 2 * cw * ch)), canvas(canvas_bytes);
    if (!read_all(in, src.data(), src.size()) || !read_all(in, canvas.data(), canvas.size())) return 2;
    fclose(in);

    // as h263mi_batch::plane_resize_dst: the pointers, and word stores only where every one of them and both pitches allow it
    std::vector<PlaneDst> dst(n);
    bool wide = pitch_y % 4 == 0 && pitch_c % 4 == 0 && ((uintptr_t)canvas.data() & 3u) == 0;
    for (uint32_t p = 0; p < n; p++) {
        for (int k = 0; k < 3; k++) {
            dst[p].p[k] = offsets[3 * p] == ~0ull || (k == 2 && nv12) ? nullptr : canvas.data() + offsets[3 * p + k];
            if (!(k == 2 && nv12)) wide = wide && (offsets[3 * p] == ~0ull || offsets[3 * p + k] % 4 == 0);
        }
    }
    std::vector<ResizeSpan> spans((size_t)ow + oh + cow + coh);
    resize_spans(w, ow, spans.data());
    resize_spans(h, oh, spans.data() + ow);
    resize_spans(cw, cow, spans.data() + ow + oh);
    resize_spans(ch, coh, spans.data() + ow + oh + cow);
    PlaneResizeArgs a{};
    a.src = src.data();
    a.dst = dst.data();
    a.cols_y = spans.data();
    a.rows_y = a.cols_y + ow;
    a.cols_c = a.rows_y + oh;
    a.rows_c = a.cols_c + cow;
    a.w = w, a.h = h, a.cw = cw, a.ch = ch;
    a.ow = ow, a.oh = oh, a.cow = cow, a.coh = coh;
    a.pitch_y = pitch_y;
    a.pitch_c = pitch_c;
    a.nv12 = nv12;
    a.wide = wide ? 1u : 0u;
    a.d_y = w * h;
    a.d_c = cw * ch;
    a.inv_d_y = 1.0f / (float)a.d_y;
    a.inv_d_c = 1.0f / (float)a.d_c;
    a.n_pictures = n;
    LaunchDims d;
    if (n) {                                             // (as launch_plane_resize: no picture, no launch)
        if (!plane_resize_plan(a, d)) return 2;
        run_banded<PlaneLds, PlaneLane>(d, a.bands, a.chunk, [&](PlaneLds &lds, uint32_t band, uint32_t z, uint32_t p, auto each) {
            plane_resize_item(a, lds, band, z, p, each);
        });
    }
    return write_canvas(argv[2], canvas);
}
