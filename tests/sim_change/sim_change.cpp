// sim_change.cpp -- CPU logic checker of k_change and k_change_select (TEST INFRASTRUCTURE).
//
// Runs change_wave and change_select (h263-rs_amd/csrc/change_kernel.inl) lane by lane: every wave of the launch (picture, cell
// row, segment), its 64 lanes one after the other in each phase, the LDS hand-off a plain struct.  cur and prev are heap buffers of
// exactly the bytes the sets name, the grids, the summaries and the list heap buffers of exactly their extents, so
// AddressSanitizer sees a read or a write one byte outside them.  Built by tests/test_sim_change.py with
// g++ -fsanitize=address,undefined into a temporary directory (the mutants of mutants.h with their -D); never part of the product.
//
//   sim_change <in> <out>
//   in : u32 w, h, n_pictures, cell_log2, roll, cell_threshold, min_changed_cells, flags (1: grids wanted, 2: list wanted,
//        4: per-picture words follow; bits 8 and up: the items a wave takes, 0 = what the launcher would choose);
//        u64 cur_offset (d_base's offset into the buffer), cur_pitch, cur_stride, cur_bytes (of the buffer), cur_set1,
//            prev_offset, prev_pitch, prev_stride, prev_bytes;
//        [n_pictures words;] cur_bytes of cur; prev_bytes of prev
//   out: prev after the launch; [n * gw * gh cell words, 0xC3C3C3C3 where the launch wrote none;] n summaries;
//        [n list words, 0xC3C3C3C3 where none was written, then the count]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../h263-rs_amd/csrc/change_kernel.inl"

using namespace h263mi;

static bool read_all(FILE *f, void *p, size_t n) { return !n || fread(p, 1, n, f) == n; }
static bool write_all(FILE *f, const void *p, size_t n) { return !n || fwrite(p, 1, n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    uint32_t hd[8];
    uint64_t q[9];
    if (!read_all(in, hd, sizeof hd) || !read_all(in, q, sizeof q)) return 2;
    const uint32_t w = hd[0], h = hd[1], n = hd[2], cl = hd[3], flags = hd[7] & 0xffu;
    if (!w || !h || !n || cl < 3 || cl > 6 || q[0] > q[3] || q[5] > q[8]) return 2;
    // (exactly as large as the data)
    std::vector<uint32_t> words(flags & 4u ? n : 0u);
    std::vector<uint8_t> cur(q[3]), prev(q[8]);
    if (!read_all(in, words.data(), 4 * words.size()) || !read_all(in, cur.data(), cur.size()) || !read_all(in, prev.data(), prev.size()))
        return 2;
    fclose(in);

    ChangeArgs a{};
    a.w = w, a.h = h;
    a.gw = ((w - 1u) >> cl) + 1u, a.gh = ((h - 1u) >> cl) + 1u;
    a.cell_log2 = cl, a.roll = hd[4], a.threshold = hd[5];
    a.n_pictures = n;
    a.segs = (w + CHANGE_SEG - 1u) / CHANGE_SEG;
    a.cur = cur.data() + q[0];
    a.cur_pitch = q[1], a.cur_stride = q[2], a.cur_set1 = q[4];
    a.prev = prev.data() + q[5];
    a.prev_pitch = q[6], a.prev_stride = q[7];
    a.cur_align = change_align(a.cur, a.cur_pitch, a.cur_stride, a.cur_set1);           // (as the entry points)
    a.prev_align = change_align(a.prev, a.prev_pitch, a.prev_stride);
    a.words = words.empty() ? nullptr : words.data();
    std::vector<uint32_t> cells(flags & 1u ? (size_t)n * a.gw * a.gh : 0u, 0xC3C3C3C3u);
    std::vector<h263mi_change_summary> summary(n);
    memset(summary.data(), 0, n * sizeof(h263mi_change_summary));                       // (the clearing in front of the launch)
    a.cells = cells.empty() ? nullptr : cells.data();
    a.summary = summary.data();

    static ChangeLds lds;
    static ChangeLane lanes[64];
    auto each = [&](auto f) {
        for (int l = 0; l < 64; l++) f(l, lanes[l]);
    };
    // the launch's waves: blockIdx.y = picture, x = the wave's run of items (launch_change's plan, the case's items per wave)
    ChangeLaunch l;
    if (!change_plan(a, l, hd[7] >> 8)) return 2;
    for (uint32_t p = 0; p < n; p++)
        for (uint32_t x = 0; x < l.waves; x++) {
            memset(&lds, 0xA5, sizeof lds);
            memset(lanes, 0x5A, sizeof lanes);
            change_wave(a, lds, p, x * a.items_per_wave, each);
        }
    std::vector<uint32_t> list(flags & 2u ? n : 0u, 0xC3C3C3C3u);
    uint32_t count = 0xC3C3C3C3u;
    if (flags & 2u) {
        ChangeSelectArgs f{summary.data(), a.words, list.data(), &count, n, hd[6]};
        memset(&lds, 0xA5, sizeof lds);
        memset(lanes, 0x5A, sizeof lanes);
        change_select(f, lds, each);
    }

    FILE *out = fopen(argv[2], "wb");
    if (!out || !write_all(out, prev.data(), prev.size()) || !write_all(out, cells.data(), 4 * cells.size()) ||
        !write_all(out, summary.data(), n * sizeof(h263mi_change_summary)))
        return 2;
    if ((flags & 2u) && (!write_all(out, list.data(), 4 * list.size()) || !write_all(out, &count, 4))) return 2;
    fclose(out);
    return 0;
}
