// sim_framed.cpp -- CPU logic checker of k_rgba_resize_framed and k_tensor_resize_framed (TEST INFRASTRUCTURE).
//
// Runs framed_resize_item (h263-rs_amd/csrc/resize_kernel.inl) and framed_tensor_item (tensor_resize_kernel.inl) lane by lane:
// every wave of the launch (band, segment, picture), its 64 lanes one after the other in each phase, the LDS hand-off a plain
// struct.  The span tables are made as the host makes them: over sw -> dw and sh -> dh, `first` offset by sx / sy.  Built by
// tests/test_sim_framed.py with g++ -fsanitize=address,undefined into a temporary directory; never part of the product.
//
//   sim_framed <in> <out>
//   in : u32 w, h, W', H', n_pictures, dtype (0..2 the tensor's, 3 = RGBA), bgr, keep_outside;
//        u32 sx, sy, sw, sh, dx, dy, dw, dh;  u32 pad (R | G << 8 | B << 16), pitch (RGBA: bytes between output rows);
//        f32 scale[3], bias[3]; u64 stride_c, stride_h (elements, spelled out), canvas_bytes;
//        u64 offsets[n_pictures] (BYTES into the canvas; ~0 = the picture is skipped);
//        n_pictures full-size pictures, w*h*4 bytes each; canvas_bytes of canvas
//   out: the canvas after the launch
#include <stdlib.h>

#include "../../h263-rs_amd/csrc/tensor_resize_kernel.inl"
#include "../sim_common.h"

using namespace h263mi;

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    uint32_t hd[8], rc[8], pp[2];
    float sb[6];
    uint64_t q[3];
    if (!read_all(in, hd, sizeof hd) || !read_all(in, rc, sizeof rc) || !read_all(in, pp, sizeof pp) || !read_all(in, sb, sizeof sb) ||
        !read_all(in, q, sizeof q))
        return 2;
    const uint32_t w = hd[0], h = hd[1], cw = hd[2], ch = hd[3], n = hd[4], dtype = hd[5];
    const uint32_t sx = rc[0], sy = rc[1], sw = rc[2], sh = rc[3], dx = rc[4], dy = rc[5], dw = rc[6], dh = rc[7];
    if (!sw || !sh || !dw || !dh || sx + sw > w || sy + sh > h || dx + dw > cw || dy + dh > ch) return 2;
    std::vector<uint64_t> offsets(n);
    if (!read_all(in, offsets.data(), 8 * (size_t)n)) return 2;
    // (exactly as large as the data: ASan sees a read or a write one byte outside)
    std::vector<uint8_t> src((size_t)n * w * h * 4), canvas(q[2]);
    if (!read_all(in, src.data(), src.size()) || !read_all(in, canvas.data(), canvas.size())) return 2;
    fclose(in);

    std::vector<uint8_t *> dst(n);
    for (uint32_t p = 0; p < n; p++) dst[p] = offsets[p] == ~0ull ? nullptr : canvas.data() + offsets[p];
    std::vector<ResizeSpan> spans((size_t)dw + dh);
    resize_spans(sw, dw, spans.data());
    resize_spans(sh, dh, spans.data() + dw);
    for (uint32_t k = 0; k < dw; k++) spans[k].first += sx;
    for (uint32_t k = 0; k < dh; k++) spans[dw + k].first += sy;
    FramedTensorArgs a{};
    ResizeArgs &r = a.t.r;
    r.src = src.data();
    r.dst = dst.data();
    r.cols = spans.data();
    r.rows = spans.data() + dw;
    r.w = w;
    r.h = h;
    r.ow = dw;
    r.oh = dh;
    r.pitch = pp[1];
    r.d = sw * sh;
    r.inv_d = 1.0f / (float)r.d;
    r.n_pictures = n;
    a.f.cw = cw, a.f.ch = ch, a.f.dx = dx, a.f.dy = dy;
    a.f.pad = pp[0];
    a.f.keep = hd[7];
    a.t.dtype = dtype;
    a.t.bgr = hd[6];
    for (int c = 0; c < 3; c++) a.t.scale[c] = sb[c], a.t.bias[c] = sb[3 + c];
    a.t.stride_c = q[0];
    a.t.stride_h = q[1];
    FramedResizeArgs ra{r, a.f};
    LaunchDims d;
    if (!n) return write_canvas(argv[2], canvas);        // (as the launchers: no picture, no launch)
    if (dtype == 3) {
        if (!framed_resize_plan(ra, d)) return 2;
        run_banded<ResizeLds, ResizeLane>(d, ra.r.bands, ra.r.chunk, [&](ResizeLds &lds, uint32_t band, uint32_t z, uint32_t p, auto each) {
            framed_resize_item(ra, lds, band, z, p, each);
        });
    } else {
        if (!framed_tensor_plan(a, d)) return 2;
        run_banded<ResizeLds, TensorLane>(d, r.bands, r.chunk, [&](ResizeLds &lds, uint32_t band, uint32_t z, uint32_t p, auto each) {
            framed_tensor_item(a, lds, band, z, p, each);
        });
    }
    return write_canvas(argv[2], canvas);
}
