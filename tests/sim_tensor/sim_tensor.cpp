// sim_tensor.cpp -- CPU logic checker of k_tensor_resize (TEST INFRASTRUCTURE).
//
// Runs tensor_resize_item of h263-rs_amd/csrc/tensor_resize_kernel.inl lane by lane: every wave of the launch (band, segment,
// picture), its 64 lanes one after the other in each phase, the LDS hand-off a plain struct.  Built by
// tests/test_sim_tensor_out.py with g++ -fsanitize=address,undefined into a temporary directory; never part of the product.
//
//   sim_tensor <in> <out>
//   in : u32 w, h, ow, oh, n_pictures, dtype, bgr, 0; f32 scale[3], bias[3]; u64 stride_c, stride_h (elements, spelled out),
//        canvas_bytes; u64 offsets[n_pictures] (BYTES into the canvas; ~0 = the picture is skipped);
//        n_pictures full-size pictures, w*h*4 bytes each; canvas_bytes of canvas
//   out: the canvas after the launch
//   sim_tensor --cvt <in> <out>
//   in : binary32 bit patterns (u32 each);  out: per pattern u16 binary16 bits, u16 bfloat16 bits -- the integer conversions
//        of the host build
#include <stdlib.h>

#include "../../h263-rs_amd/csrc/tensor_resize_kernel.inl"
#include "../sim_common.h"

using namespace h263mi;

static int convert(const char *in_path, const char *out_path)
{
    FILE *in = fopen(in_path, "rb");
    if (!in) return 2;
    fseek(in, 0, SEEK_END);
    const size_t n = (size_t)ftell(in) / 4;
    fseek(in, 0, SEEK_SET);
    std::vector<uint32_t> b(n);
    if (!read_all(in, b.data(), 4 * n)) return 2;
    fclose(in);
    std::vector<uint16_t> o(2 * n);
    for (size_t i = 0; i < n; i++) {
        o[2 * i] = (uint16_t)tensor_cvt16(TENSOR_F16, b[i]);
        o[2 * i + 1] = (uint16_t)tensor_cvt16(TENSOR_BF16, b[i]);
    }
    FILE *out = fopen(out_path, "wb");
    if (!out || fwrite(o.data(), 2, o.size(), out) != o.size()) return 2;
    fclose(out);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 4 && !strcmp(argv[1], "--cvt")) return convert(argv[2], argv[3]);
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    uint32_t hd[8];
    float sb[6];
    uint64_t q[3];
    if (!read_all(in, hd, sizeof hd) || !read_all(in, sb, sizeof sb) || !read_all(in, q, sizeof q)) return 2;
    const uint32_t w = hd[0], h = hd[1], ow = hd[2], oh = hd[3], n = hd[4];
    std::vector<uint64_t> offsets(n);
    if (!read_all(in, offsets.data(), 8 * (size_t)n)) return 2;
    // (exactly as large as the data: ASan sees a read or a write one byte outside)
    std::vector<uint8_t> src((size_t)n * w * h * 4), canvas(q[2]);
    if (!read_all(in, src.data(), src.size()) || !read_all(in, canvas.data(), canvas.size())) return 2;
    fclose(in);

    std::vector<uint8_t *> dst(n);
    for (uint32_t p = 0; p < n; p++) dst[p] = offsets[p] == ~0ull ? nullptr : canvas.data() + offsets[p];
    std::vector<ResizeSpan> spans((size_t)ow + oh);
    resize_spans(w, ow, spans.data());
    resize_spans(h, oh, spans.data() + ow);
    TensorArgs a{};
    a.r.src = src.data();
    a.r.dst = dst.data();
    a.r.cols = spans.data();
    a.r.rows = spans.data() + ow;
    a.r.w = w;
    a.r.h = h;
    a.r.ow = ow;
    a.r.oh = oh;
    a.r.d = w * h;
    a.r.inv_d = 1.0f / (float)a.r.d;
    a.r.n_pictures = n;
    a.dtype = hd[5];
    a.bgr = hd[6];
    for (int c = 0; c < 3; c++) a.scale[c] = sb[c], a.bias[c] = sb[3 + c];
    a.stride_c = q[0];
    a.stride_h = q[1];
    LaunchDims d;
    if (n) {                                             // (as launch_tensor_resize: no picture, no launch)
        if (!tensor_resize_plan(a, d)) return 2;
        run_banded<ResizeLds, TensorLane>(d, a.r.bands, a.r.chunk, [&](ResizeLds &lds, uint32_t band, uint32_t z, uint32_t p, auto each) {
            tensor_resize_item(a, lds, band, z, p, each);
        });
    }
    return write_canvas(argv[2], canvas);
}
