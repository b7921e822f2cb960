// sim_roi.cpp -- CPU logic checker of k_roi_tensor (TEST INFRASTRUCTURE).
//
// Runs roi_tensor_item (h263-rs_amd/csrc/roi_kernel.inl) lane by lane: every wave of the launch (band, segment, region), its 64
// lanes one after the other in each phase, the LDS hand-off a plain struct.  The pictures, the table and the canvas are buffers of
// exactly the bytes the caller names, so AddressSanitizer sees a read or a write one byte outside them.  Built by
// tests/test_sim_roi.py with g++ -fsanitize=address,undefined into a temporary directory; never part of the product.
//
//   sim_roi <in> <out>
//   in : u32 w, h, n_pictures, W', H', dtype (0..2), bgr, n_rois;  f32 scale[3], bias[3];
//        u64 stride_n, stride_c, stride_h (elements, spelled out), base_bytes (d_out's offset into the canvas), canvas_bytes;
//        n_rois records of 16 bytes; n_pictures full-size pictures, w*h*4 bytes each; canvas_bytes of canvas
//   out: the canvas after the launch, then n_rois status words (0xC3C3C3C3 where the launch wrote none)
//   sim_roi --spans
//        roi_span(X, size, out) == resize_spans(size, out)[X], `first` offset by an origin: every X for every (size, out) of
//        1..400 x 1..300, and with 65535 on either side; prints the mismatches, exit status 1 if any
//   sim_roi --div <d>
//        resize_div(n, d, inv) == n / d for n = q*d - 1, q*d, q*d + d/2, q = 0..255, with inv = fl(1/d), its two neighbours (a
//        reciprocal good to 1 ulp) and roi_inv_d(d); exit status 1 if any differs
#include <math.h>
#include <stdlib.h>

#include "../../h263-rs_amd/csrc/roi_kernel.inl"
#include "../sim_common.h"

using namespace h263mi;

static int bad_spans = 0;

static void check_spans(uint32_t size, uint32_t out, uint32_t origin)
{
    static std::vector<ResizeSpan> want;
    want.resize(out);
    resize_spans(size, out, want.data());
    const float inv = 1.0f / (float)out;
    for (uint32_t X = 0; X < out; X++) {
        const ResizeSpan g = roi_span(X, size, out, inv, origin), &w = want[X];
        if (g.first != w.first + origin || g.count != w.count || g.w_first != w.w_first || g.w_last != w.w_last) {
            if (bad_spans < 10)
                printf("size=%u out=%u X=%u: (%u, %u, %u, %u), want (%u, %u, %u, %u)\n", size, out, X, g.first, g.count, g.w_first, g.w_last,
                       w.first + origin, w.count, w.w_first, w.w_last);
            bad_spans++;
        }
    }
}

static int spans_main()
{
    for (uint32_t size = 1; size <= 400; size++)
        for (uint32_t out = 1; out <= 300; out++) check_spans(size, out, size & 7u);
    const uint32_t other[] = {1, 2, 3, 255, 256, 257, 4096, 32767, 32768, 65534, 65535};
    for (uint32_t o : other) {
        check_spans(65535, o, 0);
        check_spans(o, 65535, 3);
    }
    return bad_spans ? 1 : 0;
}

static int div_main(uint32_t d)
{
    const float exact = 1.0f / (float)d;
    const float invs[4] = {exact, nextafterf(exact, 0.0f), nextafterf(exact, 1.0f), roi_inv_d(d)};
    int bad = 0;
    for (float inv_d : invs)
        for (uint64_t q = 0; q <= 255; q++) {
            const uint64_t ns[3] = {q * d - (q ? 1 : 0), q * d, q * d + d / 2};
            for (uint64_t n : ns) {
                const uint32_t got = resize_div(n, d, inv_d), want = (uint32_t)(n / d);
                if (got != want) {
                    if (bad < 10) printf("d=%u inv=%a n=%llu: %u, want %u\n", d, inv_d, (unsigned long long)n, got, want);
                    bad++;
                }
            }
        }
    return bad ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "--spans")) return spans_main();
    if (argc == 3 && !strcmp(argv[1], "--div")) return div_main((uint32_t)strtoul(argv[2], nullptr, 10));
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    uint32_t hd[8];
    float sb[6];
    uint64_t q[5];
    if (!read_all(in, hd, sizeof hd) || !read_all(in, sb, sizeof sb) || !read_all(in, q, sizeof q)) return 2;
    const uint32_t w = hd[0], h = hd[1], n = hd[2], ow = hd[3], oh = hd[4], dtype = hd[5], n_rois = hd[7];
    if (!w || !h || !n || !ow || !oh || dtype > TENSOR_BF16 || q[3] > q[4]) return 2;
    // (exactly as large as the data)
    std::vector<RoiRecord> rois(n_rois);
    std::vector<uint8_t> src((size_t)n * w * h * 4), canvas(q[4]);
    std::vector<uint32_t> status(n_rois, 0xC3C3C3C3u);
    if (!read_all(in, rois.data(), 16 * (size_t)n_rois) || !read_all(in, src.data(), src.size()) || !read_all(in, canvas.data(), canvas.size()))
        return 2;
    fclose(in);

    RoiArgs a{};
    ResizeArgs &r = a.t.r;
    r.src = src.data();
    r.w = w, r.h = h, r.ow = ow, r.oh = oh;
    r.n_pictures = n;
    a.t.dtype = dtype;
    a.t.bgr = hd[6];
    for (int c = 0; c < 3; c++) a.t.scale[c] = sb[c], a.t.bias[c] = sb[3 + c];
    a.t.stride_c = q[1];
    a.t.stride_h = q[2];
    a.rois = rois.data();
    a.dst = canvas.data() + q[3];
    a.stride_n = q[0];
    a.status = status.data();
    a.n_rois = n_rois;
    a.inv_ow = 1.0f / (float)ow, a.inv_oh = 1.0f / (float)oh;
    LaunchDims d;
    if (n_rois) {                                            // (as launch_roi_tensor: no region, no launch)
        if (!roi_plan(a, d)) return 2;
        run_banded<ResizeLds, RoiLane>(d, r.bands, r.chunk, [&](ResizeLds &lds, uint32_t band, uint32_t z, uint32_t k, auto each) {
            roi_tensor_item(a, lds, band, z, k, each);
        });
    }
    return write_canvas(argv[2], canvas, status.data(), 4 * (size_t)n_rois);
}
