// sim_layout.cpp -- CPU logic checker of the scaled / pitched RGBA store of the post kernels (TEST INFRASTRUCTURE).
//
// Runs the post phases of h263-rs_amd/csrc/post_kernel.inl lane by lane, as tests/sim/sim.cpp does, with the output-layout
// fields of PostArgs set (rgba_scale, rgba_pitch) and the LAYOUT instantiations of post_phase_store.  Built by
// tests/test_sim_rgba_layout.py with g++ -fsanitize=address,undefined into a temporary directory; never part of the product.
//
//   sim_layout <in> <out>
//   in : u32 w, h, n_pictures, strength, scale, pitch; u64 canvas_bytes; u64 offsets[n_pictures];
//        n_pictures pitched frames (make_layout(w, h).frame_bytes each); canvas_bytes of canvas
//   out: the canvas after the launch
// Every picture's waves see the canvas through its own base pointer (canvas + offsets[p]), as the kernels see it through
// PostArgs::rgba_ptrs.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../h263-rs_amd/csrc/post_kernel.inl"

using namespace h263mi;

template <bool INTERIOR, int SCALE>
static void sim_tile(const PostArgs &a, PostStrip &s, PostFetch (*pf)[64], int sx, int sy0)
{
    for (int l = 0; l < 64; l++) post_phase_fetch<INTERIOR>(a, pf[0][l], l, sx, sy0, 0);
    for (int l = 0; l < 64; l++) post_phase_fetch<INTERIOR>(a, pf[1][l], l, sx, sy0 + 1, 0);
    for (int k = 0; k < POST_STRIPS; k++) {
        const int sy = sy0 + k;
        memset(&s, 0xA5, sizeof s);
        for (int l = 0; l < 64; l++) post_phase_commit<INTERIOR>(a, s, pf[k & 1][l], l);
        if (k + 2 < POST_STRIPS)
            for (int l = 0; l < 64; l++) post_phase_fetch<INTERIOR>(a, pf[k & 1][l], l, sx, sy + 2, 0);
        if (a.strength) {
            for (int l = 0; l < 64; l++) post_phase_hedges<INTERIOR>(a, s, l, sx, sy);
            for (int l = 0; l < 64; l++) post_phase_vedges<INTERIOR>(a, s, l, sx, sy);
        }
        for (int l = 0; l < 64; l++) post_phase_store<false, INTERIOR, SCALE>(a, s, l, sx, sy, 0);
    }
}

template <int SCALE>
static void sim_picture(const PostArgs &a, PostStrip &s)
{
    static PostFetch pf[2][64];
    for (int ty = 0; ty < (int)a.tiles_y; ty++)
        for (int sx = (int)a.wrap; sx < (int)(a.tiles_x + a.wrap); sx++) {
            if (post_tile_is_interior(a, sx, ty)) sim_tile<true, SCALE>(a, s, pf, sx, ty * POST_STRIPS);
            else sim_tile<false, SCALE>(a, s, pf, sx, ty * POST_STRIPS);
        }
}

static bool read_all(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    uint32_t hd[6];
    uint64_t canvas_bytes = 0;
    if (!read_all(in, hd, sizeof hd) || !read_all(in, &canvas_bytes, 8)) return 3;
    const uint32_t w = hd[0], h = hd[1], n = hd[2], strength = hd[3], scale = hd[4], pitch = hd[5];
    if (scale > 2 || !n) return 3;
    std::vector<uint64_t> offsets(n);
    if (!read_all(in, offsets.data(), 8 * n)) return 3;
    const FrameLayout L = make_layout(w, h);
    // exactly sized heap blocks: AddressSanitizer reports any byte read or written outside them
    uint8_t *frames = (uint8_t *)malloc((size_t)n * L.frame_bytes);
    uint8_t *canvas = (uint8_t *)malloc(canvas_bytes ? canvas_bytes : 1);
    if (!read_all(in, frames, (size_t)n * L.frame_bytes) || !read_all(in, canvas, canvas_bytes)) return 3;
    fclose(in);
    PostStrip *s = (PostStrip *)aligned_alloc(16, (sizeof(PostStrip) + 15) / 16 * 16);
    for (uint32_t p = 0; p < n; p++) {
        PostArgs a{};
        a.L = L;
        a.frames = frames + (size_t)p * L.frame_bytes;
        a.rgba = canvas + offsets[p];
        a.n_pictures = 1;
        a.strength = strength;
        a.tiles_x = post_tile_columns(a.L.width, &a.wrap);      // as host_common.h: set_post_tiles
        a.tiles_y = (post_strips_y(h) + POST_STRIPS - 1) / POST_STRIPS;
        a.rgba_scale = scale;
        a.rgba_pitch = pitch;
        if (scale == 0) sim_picture<0>(a, *s);
        else if (scale == 1) sim_picture<1>(a, *s);
        else sim_picture<2>(a, *s);
    }
    free(s);
    FILE *out = fopen(argv[2], "wb");
    if (!out || fwrite(canvas, 1, canvas_bytes, out) != canvas_bytes) return 4;
    fclose(out);
    free(frames);
    free(canvas);
    return 0;
}
