// sim_filter.cpp -- CPU logic checker of k_rgba_filter and k_tensor_filter (TEST INFRASTRUCTURE).
//
// Runs filter_rgba_item and filter_tensor_item (h263-rs_amd/csrc/filter_kernel.inl) lane by lane: every wave of the launch (band,
// segment, picture), its 64 lanes one after the other in each phase, the LDS a plain struct.  The tap tables are made as the host
// makes them (filter_taps.h: filter_table).  Built by tests/test_sim_filter.py with g++ -fsanitize=address,undefined
// -ffp-contract=off into a temporary directory -- also with -DH263MI_MUTATE_FILTER_SINGLE_ROUNDING and with
// -DH263MI_MUTATE_FILTER_NO_CLAMP, which must fail --; never part of the product.
//
//   sim_filter <in> <out>
//   in : u32 w, h, W', H', n_pictures, dtype (0..2 the tensor's, 3 = RGBA), bgr, keep_outside;
//        u32 sx, sy, sw, sh, dx, dy, dw, dh;  u32 pad (R | G << 8 | B << 16), pitch (RGBA: bytes between output rows), kind, 0;
//        f32 scale[3], bias[3]; u64 stride_c, stride_h (elements, spelled out), canvas_bytes;
//        u64 offsets[n_pictures] (BYTES into the canvas; ~0 = the picture is skipped);
//        n_pictures full-size pictures, w*h*4 bytes each; canvas_bytes of canvas
//   out: the canvas after the launch
#include <stdlib.h>

#include "../../h263-rs_amd/csrc/filter_kernel.inl"
#include "../../h263-rs_amd/csrc/filter_taps.h"
#include "../sim_common.h"

using namespace h263mi;

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    uint32_t hd[8], rc[8], pp[4];
    float sb[6];
    uint64_t q[3];
    if (!read_all(in, hd, sizeof hd) || !read_all(in, rc, sizeof rc) || !read_all(in, pp, sizeof pp) || !read_all(in, sb, sizeof sb) ||
        !read_all(in, q, sizeof q))
        return 2;
    const uint32_t w = hd[0], h = hd[1], cw = hd[2], ch = hd[3], n = hd[4], dtype = hd[5], kind = pp[2];
    const uint32_t sx = rc[0], sy = rc[1], sw = rc[2], sh = rc[3], dx = rc[4], dy = rc[5], dw = rc[6], dh = rc[7];
    if (!sw || !sh || !dw || !dh || sx + sw > w || sy + sh > h || dx + dw > cw || dy + dh > ch) return 2;
    if (kind != FILTER_BILINEAR && kind != FILTER_BICUBIC) return 2;
    std::vector<uint64_t> offsets(n);
    if (!read_all(in, offsets.data(), 8 * (size_t)n)) return 2;
    // (exactly as large as the data: ASan sees a read or a write one byte outside)
    std::vector<uint8_t> src((size_t)n * w * h * 4), canvas(q[2]);
    if (!read_all(in, src.data(), src.size()) || !read_all(in, canvas.data(), canvas.size())) return 2;
    fclose(in);

    std::vector<uint8_t *> dst(n);
    for (uint32_t p = 0; p < n; p++) dst[p] = offsets[p] == ~0ull ? nullptr : canvas.data() + offsets[p];
    const FilterTable table = filter_table(kind, sx, sy, sw, sh, dw, dh);
    TensorFilterArgs a{};
    FilterArgs &r = a.fl;
    r.src = src.data();
    r.dst = dst.data();
    filter_axes(table.words.data(), dw, dh, table.ksx, table.ksy, r.x, r.y);
    r.w = w;
    r.h = h;
    r.dw = dw;
    r.dh = dh;
    r.pitch = pp[1];
    r.n_pictures = n;
    r.f.cw = cw, r.f.ch = ch, r.f.dx = dx, r.f.dy = dy;
    r.f.pad = pp[0];
    r.f.keep = hd[7];
    a.t.dtype = dtype;
    a.t.bgr = hd[6];
    for (int c = 0; c < 3; c++) a.t.scale[c] = sb[c], a.t.bias[c] = sb[3 + c];
    a.t.stride_c = q[0];
    a.t.stride_h = q[1];
    LaunchDims d;
    if (!n) return write_canvas(argv[2], canvas);        // (as the launchers: no picture, no launch)
    if (dtype == 3) {
        if (!filter_rgba_plan(r, d)) return 2;
        run_banded<FilterLds, FilterLane>(d, r.bands, r.chunk, [&](FilterLds &lds, uint32_t band, uint32_t z, uint32_t p, auto each) {
            filter_rgba_item(r, lds, band, z, p, each);
        });
    } else {
        if (!filter_tensor_plan(a, d)) return 2;
        run_banded<FilterLds, TensorFilterLane>(d, r.bands, r.chunk, [&](FilterLds &lds, uint32_t band, uint32_t z, uint32_t p, auto each) {
            filter_tensor_item(a, lds, band, z, p, each);
        });
    }
    return write_canvas(argv[2], canvas);
}
