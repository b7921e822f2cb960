// sim_bg.cpp -- CPU logic checker of k_bg_begin, k_bg and the selection behind them (TEST INFRASTRUCTURE).
//
// Runs bg_begin, bg_wave (h263-rs_amd/csrc/background_kernel.inl) and change_select lane by lane: every lane of k_bg_begin, then
// every wave of the launch that bg_plan lays out (picture, cell row, segment), its 64 lanes one after the other in each phase, the
// LDS hand-off a plain struct.  cur, the mask and the cut list are heap buffers of exactly the bytes the call may touch, the state,
// the grids, the summaries and the list heap buffers of exactly their extents, so AddressSanitizer sees a read or a write one byte
// outside them.  Built by tests/test_sim_bg.py with g++ -fsanitize=address,undefined into a temporary directory (the mutants of
// mutants.h with their -D); never part of the product.
//
//   sim_bg <in> <out>
//   in : u32 w, h, n_pictures, cell_log2, learn_shift, fg_learn_shift, pixel_threshold, warmup, cell_threshold, min_changed_cells,
//            flags (1: grids wanted, 2: list wanted, 4: per-picture words follow, 8: a cut list follows, 16: a mask follows; bits 8
//            and up: the items a wave takes, 0 = what the launcher would choose), cut_count (the count word), cut_words (entries
//            that follow), three reserved;
//        u64 cur_offset (d_base's offset into the buffer), cur_pitch, cur_stride, cur_bytes (of the buffer), cur_set1,
//            mask_offset, mask_pitch, mask_stride, mask_bytes;
//        [n_pictures words;] [cut_words entries;] the state; cur_bytes of cur; [mask_bytes of the mask]
//   out: the state after the call; [the mask;] [n * gw * gh cell words, 0xC3C3C3C3 where the launch wrote none;] n summaries
//        (0xC3 bytes where the launch wrote none); [n list words, 0xC3C3C3C3 where none was written, then the count]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../h263-rs_amd/csrc/background_kernel.inl"

using namespace h263mi;

static bool read_all(FILE *f, void *p, size_t n) { return !n || fread(p, 1, n, f) == n; }
static bool write_all(FILE *f, const void *p, size_t n) { return !n || fwrite(p, 1, n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    uint32_t hd[16];
    uint64_t q[9];
    if (!read_all(in, hd, sizeof hd) || !read_all(in, q, sizeof q)) return 2;
    const uint32_t w = hd[0], h = hd[1], n = hd[2], cl = hd[3], flags = hd[10] & 0xffu;
    if (!w || !h || !n || cl < 3 || cl > 6 || q[0] > q[3] || q[5] > q[8]) return 2;
    // (exactly as large as the data; the state 32-byte aligned, as the entry points demand)
    const size_t state_bytes = (size_t)n * bg_stride(w, h);
    std::vector<uint32_t> words(flags & 4u ? n : 0u), cut(flags & 8u ? hd[12] : 0u);
    uint32_t *const cut_count = flags & 8u ? new uint32_t(hd[11]) : nullptr;
    uint8_t *const state = static_cast<uint8_t *>(aligned_alloc(32, state_bytes));
    std::vector<uint8_t> cur(q[3]), mask(flags & 16u ? q[8] : 0u);
    if (!state || !read_all(in, words.data(), 4 * words.size()) || !read_all(in, cut.data(), 4 * cut.size()) ||
        !read_all(in, state, state_bytes) || !read_all(in, cur.data(), cur.size()) || !read_all(in, mask.data(), mask.size()))
        return 2;
    fclose(in);

    BgArgs a{};
    a.w = w, a.h = h;
    a.gw = ((w - 1u) >> cl) + 1u, a.gh = ((h - 1u) >> cl) + 1u;
    a.cell_log2 = cl, a.threshold = hd[8];
    a.learn_shift = hd[4], a.fg_learn_shift = hd[5], a.pixel_threshold = hd[6], a.warmup = hd[7];
    a.n_pictures = n;
    a.segs = (w + CHANGE_SEG - 1u) / CHANGE_SEG;
    a.bpitch = bg_pitch(w), a.state_stride = bg_stride(w, h);
    a.state = state;
    a.cur = cur.data() + q[0];
    a.cur_pitch = q[1], a.cur_stride = q[2], a.cur_set1 = q[4];
    a.cur_align = change_align(a.cur, a.cur_pitch, a.cur_stride, a.cur_set1);           // (as the entry points)
    if (flags & 16u) {
        a.mask = mask.data() + q[5];
        a.mask_pitch = q[6], a.mask_stride = q[7];
        a.mask_align = change_align(a.mask, a.mask_pitch, a.mask_stride);
    }
    a.words = words.empty() ? nullptr : words.data();
    // (an empty list still has a pointer: the count says that nothing of it is read)
    static uint32_t nothing;
    a.cut = flags & 8u ? (cut.empty() ? &nothing : cut.data()) : nullptr;
    a.cut_count = cut_count;
    std::vector<uint32_t> cells(flags & 1u ? (size_t)n * a.gw * a.gh : 0u, 0xC3C3C3C3u);
    std::vector<h263mi_change_summary> summary(n);
    memset(summary.data(), 0xC3, n * sizeof(h263mi_change_summary));                    // (k_bg_begin clears them)
    a.cells = cells.empty() ? nullptr : cells.data();
    a.summary = summary.data();

    static ChangeLds lds;
    static ChangeLane lanes[64];
    auto each = [&](auto f) {
        for (int l = 0; l < 64; l++) f(l, lanes[l]);
    };
    // the launches: k_bg_begin's lanes, then k_bg's waves -- blockIdx.y = picture, x = the wave's run of items (launch_background's
    // plan, the case's items per wave)
    BgLaunch l;
    if (!bg_plan(a, l, hd[10] >> 8)) return 2;
    for (uint32_t p = 0; p < n; p++) bg_begin(a, p);
    for (uint32_t p = 0; p < n; p++)
        for (uint32_t x = 0; x < l.waves; x++) {
            memset(&lds, 0xA5, sizeof lds);
            memset(lanes, 0x5A, sizeof lanes);
            bg_wave(a, lds, p, x * a.items_per_wave, each);
        }
    std::vector<uint32_t> list(flags & 2u ? n : 0u, 0xC3C3C3C3u);
    uint32_t count = 0xC3C3C3C3u;
    if (flags & 2u) {
        ChangeSelectArgs f{summary.data(), a.words, list.data(), &count, n, hd[9]};
        memset(&lds, 0xA5, sizeof lds);
        memset(lanes, 0x5A, sizeof lanes);
        change_select(f, lds, each);
    }

    FILE *out = fopen(argv[2], "wb");
    if (!out || !write_all(out, state, state_bytes) || !write_all(out, mask.data(), mask.size()) ||
        !write_all(out, cells.data(), 4 * cells.size()) || !write_all(out, summary.data(), n * sizeof(h263mi_change_summary)))
        return 2;
    if ((flags & 2u) && (!write_all(out, list.data(), 4 * list.size()) || !write_all(out, &count, 4))) return 2;
    fclose(out);
    free(state);
    delete cut_count;
    return 0;
}
