// sim_regions.cpp -- CPU logic checker of k_regions and k_regions_pack (TEST INFRASTRUCTURE).
//
// Runs regions_picture and regions_pack (h263-rs_amd/csrc/regions_kernel.inl) thread by thread: every workgroup of the launch (one a
// picture), its 1024 threads one after the other in each phase, the LDS a plain struct; then the one wave of the pack kernel.  The
// grids, the summaries, the staging area, the table, the stats, the info and the counts are heap buffers of exactly their extents,
// so AddressSanitizer sees a read or a write one byte outside them; the outputs are pre-filled with 0xC3, so a byte that the launch
// must not write keeps it.  Built by tests/test_sim_regions.py with g++ -fsanitize=address,undefined into a temporary directory
// (the mutants of mutants.h with their -D); never part of the product.
//
//   sim_regions <in> <out>
//   in : u32 w, h, n_pictures, cell_log2, connectivity, margin_cells, cell_threshold, min_cells, max_per_picture, max_rois,
//        flags (1: n summaries follow, 2: stats wanted), order (the turn of a workgroup's threads within a phase: 0 ascending,
//        1 descending, 2 scattered -- the device may take any);
//        [n summaries of 16 bytes;] n * gw * gh cell words
//   out: max_rois entries of 16 bytes; [max_rois stats of 16 bytes;] n infos of 16 bytes; the two count words
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../h263-rs_amd/csrc/regions_kernel.inl"

using namespace h263mi;

static bool read_all(FILE *f, void *p, size_t n) { return !n || fread(p, 1, n, f) == n; }
static bool write_all(FILE *f, const void *p, size_t n) { return !n || fwrite(p, 1, n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    uint32_t hd[12];
    if (!read_all(in, hd, sizeof hd)) return 2;
    const uint32_t w = hd[0], h = hd[1], n = hd[2], cl = hd[3], max_per = hd[8], max_rois = hd[9], flags = hd[10], order = hd[11];
    if (!w || !h || w > 65535 || h > 65535 || cl < 3 || cl > 6 || !max_per || max_per > REGIONS_MAX_PER_PICTURE || !max_rois ||
        max_rois > REGIONS_MAX_ROIS || n > CHANGE_MAX_PICTURES)
        return 2;
    const uint32_t gw = ((w - 1u) >> cl) + 1u, gh = ((h - 1u) >> cl) + 1u;
    if ((uint64_t)gw * gh > REGIONS_MAX_CELLS) return 2;
    // (exactly as large as the data)
    std::vector<h263mi_change_summary> summary(flags & 1u ? n : 0u);
    std::vector<uint32_t> cells((size_t)n * gw * gh);
    if (!read_all(in, summary.data(), summary.size() * sizeof(h263mi_change_summary)) || !read_all(in, cells.data(), 4 * cells.size())) return 2;
    fclose(in);
    std::vector<uint64_t> work((size_t)n * max_per * REGIONS_ENTRY / 8u);
    std::vector<h263mi_roi> rois(max_rois);
    std::vector<h263mi_region_stat> stats(flags & 2u ? max_rois : 0u);
    std::vector<h263mi_region_info> info(n);
    std::vector<uint32_t> count(2);
    if (!work.empty()) memset(work.data(), 0xC3, work.size() * 8u);
    memset(rois.data(), 0xC3, rois.size() * sizeof(h263mi_roi));
    if (!stats.empty()) memset(stats.data(), 0xC3, stats.size() * sizeof(h263mi_region_stat));
    if (!info.empty()) memset(info.data(), 0xC3, info.size() * sizeof(h263mi_region_info));
    memset(count.data(), 0xC3, 8);

    RegionsArgs a{};
    a.cells = n ? cells.data() : nullptr;
    a.summary = summary.empty() ? nullptr : summary.data();
    a.work = reinterpret_cast<uint8_t *>(work.data());
    a.info = info.data();
    a.w = w, a.h = h, a.gw = gw, a.gh = gh;
    a.cell_log2 = cl, a.connectivity = hd[4], a.margin = hd[5], a.threshold = hd[6];
    a.min_cells = hd[7], a.max_per = max_per, a.n_pictures = n;

    static RegionsLds lds;
    static RegionsLane threads[REGIONS_THREADS];
    auto each = [&](auto f) {
        for (int k = 0; k < (int)REGIONS_THREADS; k++) {
            const int t = order == 0 ? k : (order == 1 ? (int)REGIONS_THREADS - 1 - k : k * 389 % (int)REGIONS_THREADS);
            f(t, threads[t]);
        }
    };
    for (uint32_t p = 0; p < n; p++) {                     // blockIdx.x = picture
        memset(&lds, 0xA5, sizeof lds);
        memset(threads, 0x5A, sizeof threads);
        regions_picture(a, lds, p, each);
    }
    const RegionsPackArgs f{a.summary, a.work, rois.data(), stats.empty() ? nullptr : stats.data(), info.data(), count.data(),
                            n, max_per, max_rois, 0};
    static RegionsPackLds plds;
    static RegionsPackLane lanes[64];
    memset(&plds, 0xA5, sizeof plds);
    memset(lanes, 0x5A, sizeof lanes);
    regions_pack(f, plds, [&](auto g) {
        for (int l = 0; l < 64; l++) g(l, lanes[l]);
    });

    FILE *out = fopen(argv[2], "wb");
    if (!out || !write_all(out, rois.data(), rois.size() * sizeof(h263mi_roi)) ||
        !write_all(out, stats.data(), stats.size() * sizeof(h263mi_region_stat)) ||
        !write_all(out, info.data(), info.size() * sizeof(h263mi_region_info)) || !write_all(out, count.data(), 8))
        return 2;
    fclose(out);
    return 0;
}
