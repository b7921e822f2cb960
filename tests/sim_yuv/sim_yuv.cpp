// sim_yuv.cpp -- CPU logic checker of the plane store of the YUV instantiations of the post kernels (TEST INFRASTRUCTURE).
//
// Runs the post phases of h263-rs_amd/csrc/post_kernel.inl lane by lane, as tests/sim_layout/sim_layout.cpp does, with the
// YUV instantiations of post_phase_store (post_store_yuv) and the interior test they use (post_tile_is_interior_yuv).  Built
// by tests/test_sim_yuv_layout.py with g++ -fsanitize=address,undefined into a temporary directory; never part of the product.
//
//   sim_yuv <in> <out>
//   in : u32 w, h, n_pictures, strength, format (1 = I420, 2 = NV12), pitch_y, pitch_c, wide; u64 canvas_bytes;
//        u64 offsets[3 * n_pictures] (Y, Cb or CbCr, Cr per picture);
//        n_pictures pitched frames (make_layout(w, h).frame_bytes each); canvas_bytes of canvas
//   out: the canvas after the launch
// Prints the number of tiles that took the interior path.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../h263-rs_amd/csrc/post_kernel.inl"

using namespace h263mi;

template <bool INTERIOR, int FMT>
static void sim_tile(const PostArgs &a, const YuvOut &yo, PostStrip &s, PostFetch (*pf)[64], int sx, int sy0, int pic)
{
    for (int l = 0; l < 64; l++) post_phase_fetch<INTERIOR>(a, pf[0][l], l, sx, sy0, pic);
    for (int l = 0; l < 64; l++) post_phase_fetch<INTERIOR>(a, pf[1][l], l, sx, sy0 + 1, pic);
    for (int k = 0; k < POST_STRIPS; k++) {
        const int sy = sy0 + k;
        memset(&s, 0xA5, sizeof s);
        for (int l = 0; l < 64; l++) post_phase_commit<INTERIOR>(a, s, pf[k & 1][l], l);
        if (k + 2 < POST_STRIPS)
            for (int l = 0; l < 64; l++) post_phase_fetch<INTERIOR>(a, pf[k & 1][l], l, sx, sy + 2, pic);
        if (a.strength) {
            for (int l = 0; l < 64; l++) post_phase_hedges<INTERIOR>(a, s, l, sx, sy);
            for (int l = 0; l < 64; l++) post_phase_vedges<INTERIOR>(a, s, l, sx, sy);
        }
        for (int l = 0; l < 64; l++) post_phase_store<false, INTERIOR, -1, FMT>(a, s, l, sx, sy, pic, yo);
    }
}

template <int FMT>
static unsigned sim_picture(const PostArgs &a, const YuvOut &yo, PostStrip &s, int pic)
{
    static PostFetch pf[2][64];
    unsigned interior = 0;
    for (int ty = 0; ty < (int)a.tiles_y; ty++)
        for (int sx = (int)a.wrap; sx < (int)(a.tiles_x + a.wrap); sx++) {
            if (post_tile_is_interior_yuv(a, yo, sx, ty)) {
                sim_tile<true, FMT>(a, yo, s, pf, sx, ty * POST_STRIPS, pic);
                interior++;
            } else {
                sim_tile<false, FMT>(a, yo, s, pf, sx, ty * POST_STRIPS, pic);
            }
        }
    return interior;
}

static bool read_all(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    uint32_t hd[8];
    uint64_t canvas_bytes = 0;
    if (!read_all(in, hd, sizeof hd) || !read_all(in, &canvas_bytes, 8)) return 3;
    const uint32_t w = hd[0], h = hd[1], n = hd[2], strength = hd[3], format = hd[4];
    if ((format != YUV_OUT_I420 && format != YUV_OUT_NV12) || !n) return 3;
    std::vector<uint64_t> offsets((size_t)3 * n);
    if (!read_all(in, offsets.data(), 8 * offsets.size())) return 3;
    const FrameLayout L = make_layout(w, h);
    // exactly sized heap blocks: AddressSanitizer reports any byte read or written outside them
    uint8_t *frames = (uint8_t *)malloc((size_t)n * L.frame_bytes);
    uint8_t *canvas = (uint8_t *)malloc(canvas_bytes ? canvas_bytes : 1);
    if (!read_all(in, frames, (size_t)n * L.frame_bytes) || !read_all(in, canvas, canvas_bytes)) return 3;
    fclose(in);
    PostStrip *s = (PostStrip *)aligned_alloc(16, (sizeof(PostStrip) + 15) / 16 * 16);
    PostArgs a{};
    a.L = L;
    a.frames = frames;
    a.planes_out = canvas;
    a.n_pictures = n;
    a.strength = strength;
    a.tiles_x = post_tile_columns(a.L.width, &a.wrap);      // as host_common.h: set_post_tiles
    a.tiles_y = (post_strips_y(h) + POST_STRIPS - 1) / POST_STRIPS;
    YuvOut yo{};
    yo.format = format;
    yo.pitch_y = hd[5];
    yo.pitch_c = hd[6];
    yo.wide = hd[7];
    yo.offsets = offsets.data();
    unsigned interior = 0;
    for (uint32_t p = 0; p < n; p++)
        interior += format == YUV_OUT_NV12 ? sim_picture<(int)YUV_OUT_NV12>(a, yo, *s, (int)p) : sim_picture<(int)YUV_OUT_I420>(a, yo, *s, (int)p);
    free(s);
    printf("%u\n", interior);
    FILE *out = fopen(argv[2], "wb");
    if (!out || fwrite(canvas, 1, canvas_bytes, out) != canvas_bytes) return 4;
    fclose(out);
    free(frames);
    free(canvas);
    return 0;
}
