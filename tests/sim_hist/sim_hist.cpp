// sim_hist.cpp -- CPU logic checker of k_hist, k_hist_final and k_hist_select (TEST INFRASTRUCTURE).
//
// Runs hist_wave, hist_final and hist_select (h263-rs_amd/csrc/hist_kernel.inl) lane by lane: every wave of the launches that
// hist_plan describes (picture, run of work items), its 64 lanes one after the other in each phase, the LDS hand-off a plain
// struct.  The planes are a heap buffer of exactly the bytes the set names, the histograms, prev, the statistics and the list heap
// buffers of exactly their extents, so AddressSanitizer sees a read or a write one byte outside them.  Built by
// tests/test_sim_hist.py with g++ -fsanitize=address,undefined into a temporary directory (the mutants of mutants.h with their -D);
// never part of the product.
//
//   sim_hist <in> <out>
//   in : u32 w, h, n_pictures, roll, lo_permille, hi_permille, cut_permille, flags (1: prev follows, 2: list wanted, 4: per-picture
//        words follow), items a wave takes (0 = what the launcher would choose), 3 x 0;
//        u64 offset (d_base's offset into the buffer), pitch, stride, bytes (of the buffer), set1;
//        [n_pictures words;] `bytes` of planes; [n_pictures * 256 words of prev]
//   out: n * 256 histogram words; [prev after the launches;] n statistics; [n list words, 0xC3C3C3C3 where none was written, then
//        the count]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../h263-rs_amd/csrc/hist_kernel.inl"

using namespace h263mi;

static bool read_all(FILE *f, void *p, size_t n) { return !n || fread(p, 1, n, f) == n; }
static bool write_all(FILE *f, const void *p, size_t n) { return !n || fwrite(p, 1, n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    uint32_t hd[12];
    uint64_t q[5];
    if (!read_all(in, hd, sizeof hd) || !read_all(in, q, sizeof q)) return 2;
    const uint32_t w = hd[0], h = hd[1], n = hd[2], flags = hd[7];
    if (!w || !h || !n || q[0] > q[3]) return 2;
    // (exactly as large as the data)
    std::vector<uint32_t> words(flags & 4u ? n : 0u);
    std::vector<uint8_t> planes(q[3]);
    std::vector<uint32_t> prev(flags & 1u ? (size_t)n * 256u : 0u);
    if (!read_all(in, words.data(), 4 * words.size()) || !read_all(in, planes.data(), planes.size()) || !read_all(in, prev.data(), 4 * prev.size()))
        return 2;
    fclose(in);

    std::vector<uint32_t> hist((size_t)n * 256u, 0u);                                   // (the clearing in front of the launch)
    std::vector<h263mi_hist_stats> stats(n);
    memset(stats.data(), 0xC3, n * sizeof(h263mi_hist_stats));
    HistArgs a{};
    a.src = planes.data() + q[0];
    a.pitch = q[1], a.stride = q[2], a.set1 = q[4];
    a.words = words.empty() ? nullptr : words.data();
    a.hist = hist.data();
    a.w = w, a.h = h, a.n_pictures = n;
    a.align = change_align(a.src, a.pitch, a.stride, a.set1);                           // (as the entry points)
    a.segs = (w + HIST_SEG - 1u) / HIST_SEG;
    a.bands = (h + HIST_ROWS - 1u) / HIST_ROWS;

    static HistLds lds;
    static HistFinalLds flds;
    static HistLane lanes[64];
    auto each = [&](auto f) {
        for (int l = 0; l < 64; l++) f(l, lanes[l]);
    };
    // the launch's waves: blockIdx.y = picture, x = the wave's run of items (launch_hist's plan, the case's items per wave)
    HistLaunch l;
    if (!hist_plan(a, l, hd[8])) return 2;
    for (uint32_t p = 0; p < n; p++)
        for (uint32_t x = 0; x < l.waves; x++) {
            memset(&lds, 0xA5, sizeof lds);
            memset(lanes, 0x5A, sizeof lanes);
            hist_wave(a, lds, p, x * a.items_per_wave, each);
        }
    const HistFinalArgs fin{hist.data(), prev.empty() ? nullptr : prev.data(), stats.data(), a.words, (uint64_t)w * h, n, hd[4], hd[5], hd[3]};
    for (uint32_t p = 0; p < n; p++) {
        memset(&flds, 0xA5, sizeof flds);
        memset(lanes, 0x5A, sizeof lanes);
        hist_final(fin, flds, p, each);
    }
    std::vector<uint32_t> list(flags & 2u ? n : 0u, 0xC3C3C3C3u);
    uint32_t count = 0xC3C3C3C3u;
    if (flags & 2u) {
        const HistSelectArgs f{stats.data(), a.words, list.data(), &count, (uint64_t)w * h, n, hd[6]};
        memset(&flds, 0xA5, sizeof flds);
        memset(lanes, 0x5A, sizeof lanes);
        hist_select(f, flds, each);
    }

    FILE *out = fopen(argv[2], "wb");
    if (!out || !write_all(out, hist.data(), 4 * hist.size()) || !write_all(out, prev.data(), 4 * prev.size()) ||
        !write_all(out, stats.data(), n * sizeof(h263mi_hist_stats)))
        return 2;
    if ((flags & 2u) && (!write_all(out, list.data(), 4 * list.size()) || !write_all(out, &count, 4))) return 2;
    fclose(out);
    return 0;
}
