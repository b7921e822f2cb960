// sim_plane_filter.cpp -- CPU logic checker of k_plane_filter (TEST INFRASTRUCTURE).
//
// Runs plane_filter_item of h263-rs_amd/csrc/plane_filter_kernel.inl lane by lane: every wave of the launch (band, segment,
// picture), its 64 lanes one after the other in each phase, the LDS a plain struct.  The tap tables are made as the host makes
// them (filter_taps.h: filter_table, luma then chroma).  Built by tests/test_sim_plane_filter.py with g++
// -fsanitize=address,undefined -ffp-contract=off into a temporary directory -- also with -DH263MI_MUTATE_FILTER_SINGLE_ROUNDING
// and with -DH263MI_MUTATE_FILTER_NO_CLAMP, which must fail --; never part of the product.
//
//   sim_plane_filter <in> <out>
//   in : u32 w, h, ow, oh, n_pictures, nv12, pitch_y, pitch_c; u32 kind, base, 0, 0; u64 canvas_bytes;
//        u64 offsets[3 * n_pictures] (Y, Cb or CbCr, Cr, from canvas + base -- the d_deblocked of the call; Y = ~0: the picture
//        is skipped); n_pictures tight I420 pictures, w*h + 2*cw*ch bytes each; canvas_bytes of canvas
//   out: the canvas after the launch
#include <stdlib.h>

#include "../../h263-rs_amd/csrc/filter_taps.h"
#include "../../h263-rs_amd/csrc/plane_filter_kernel.inl"
#include "../sim_common.h"

using namespace h263mi;

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    uint32_t hd[8], pp[4];
    uint64_t canvas_bytes = 0;
    if (!read_all(in, hd, sizeof hd) || !read_all(in, pp, sizeof pp) || !read_all(in, &canvas_bytes, 8)) return 2;
    const uint32_t w = hd[0], h = hd[1], ow = hd[2], oh = hd[3], n = hd[4], nv12 = hd[5], pitch_y = hd[6], pitch_c = hd[7];
    const uint32_t kind = pp[0], base = pp[1];
    const uint32_t cw = (w + 1) / 2, ch = (h + 1) / 2, cow = (ow + 1) / 2, coh = (oh + 1) / 2;
    if (kind != FILTER_BILINEAR && kind != FILTER_BICUBIC) return 2;
    std::vector<uint64_t> offsets(3 * (size_t)n);
    if (!read_all(in, offsets.data(), 8 * offsets.size())) return 2;
    // (exactly as large as the data: ASan sees a read or a write one byte outside; operator new aligns both to 16 bytes)
    std::vector<uint8_t> src((size_t)n * (w * h + 2 * cw * ch)), canvas(canvas_bytes);
    if (!read_all(in, src.data(), src.size()) || !read_all(in, canvas.data(), canvas.size())) return 2;
    fclose(in);

    // as h263mi_batch::plane_resize_dst: the pointers, and word stores only where every offset, both pitches and d_deblocked allow it
    uint8_t *const d_planes = canvas.data() + base;
    std::vector<PlaneDst> dst(n);
    bool wide = pitch_y % 4 == 0 && pitch_c % 4 == 0 && ((uintptr_t)d_planes & 3u) == 0;
    for (uint32_t p = 0; p < n; p++) {
        for (int k = 0; k < 3; k++) {
            dst[p].p[k] = offsets[3 * p] == ~0ull || (k == 2 && nv12) ? nullptr : d_planes + offsets[3 * p + k];
            if (!(k == 2 && nv12)) wide = wide && (offsets[3 * p] == ~0ull || offsets[3 * p + k] % 4 == 0);
        }
    }
    // as make_yuv_resize_shape: the luma table, then the chroma table
    const FilterTable ty = filter_table(kind, 0, 0, w, h, ow, oh), tc = filter_table(kind, 0, 0, cw, ch, cow, coh);
    std::vector<uint32_t> words(ty.words);
    words.insert(words.end(), tc.words.begin(), tc.words.end());
    PlaneFilterArgs a{};
    a.src = src.data();
    a.dst = dst.data();
    a.w = w, a.h = h, a.cw = cw, a.ch = ch;
    a.ow = ow, a.oh = oh, a.cow = cow, a.coh = coh;
    plane_filter_axes(words.data(), a, ty.ksx, ty.ksy, tc.ksx, tc.ksy);
    a.pitch_y = pitch_y;
    a.pitch_c = pitch_c;
    a.nv12 = nv12;
    a.wide = wide ? 1u : 0u;
    a.d_y = w * h;
    a.d_c = cw * ch;
    a.n_pictures = n;
    LaunchDims d;
    if (n) {                                             // (as launch_plane_filter: no picture, no launch)
        if (!plane_filter_plan(a, d)) return 2;
        run_banded<PlaneFilterLds, PlaneFilterLane>(d, a.bands, a.chunk, [&](PlaneFilterLds &lds, uint32_t band, uint32_t z, uint32_t p, auto each) {
            plane_filter_item(a, lds, band, z, p, each);
        });
    }
    return write_canvas(argv[2], canvas);
}
