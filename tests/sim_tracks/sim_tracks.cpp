// sim_tracks.cpp -- CPU logic checker of k_tracks and k_tracks_pack (TEST INFRASTRUCTURE).
//
// Runs tracks_picture and tracks_pack (h263-rs_amd/csrc/tracks_kernel.inl) thread by thread: every workgroup of the launch (one a
// picture), its 256 threads one after the other in each phase, the LDS a plain struct; then the one wave of the pack kernel -- call
// after call of a sequence over one state.  The table of boxes, its infos, the cut list, the state, the output table, the refs, the
// infos and the counts are heap buffers of exactly their extents, so AddressSanitizer sees a read or a write one byte outside them;
// the outputs are pre-filled with 0xC3 before every call, so a byte that the launch must not write keeps it.  Built by
// tests/test_sim_tracks.py with g++ -fsanitize=address,undefined into a temporary directory (the mutants of mutants.h with their
// -D); never part of the product.
//
//   sim_tracks <in> <out>
//   in : u32 w, h, n_pictures, max_tracks, iou_permille, max_missed, min_hits, emit_period, max_out, flags (1: refs wanted),
//        order (the turn of a workgroup's threads within a phase: 0 ascending, 1 descending, 2 scattered), n_calls;
//        the first state, n_pictures * (32 + 32 * max_tracks) bytes;
//        per call: u32 n_rois, has_cut, cut_words, cut_count; n_rois entries of 16 bytes; n_pictures infos of 16 bytes; cut_words words
//   out: per call: the state; max_out entries of 16 bytes; [max_out refs of 16 bytes;] n_pictures infos of 32 bytes; the two count words
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../h263-rs_amd/csrc/tracks_kernel.inl"

using namespace h263mi;

static bool read_all(FILE *f, void *p, size_t n) { return !n || fread(p, 1, n, f) == n; }
static bool write_all(FILE *f, const void *p, size_t n) { return !n || fwrite(p, 1, n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    FILE *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t hd[12];
    if (!read_all(in, hd, sizeof hd)) return 2;
    const uint32_t w = hd[0], h = hd[1], n = hd[2], max_tracks = hd[3], max_out = hd[8], flags = hd[9], order = hd[10], n_calls = hd[11];
    if (!w || !h || w > 65535 || h > 65535 || !max_tracks || max_tracks > TRACKS_MAX || !max_out || max_out > TRACKS_MAX_OUT ||
        n > TRACKS_MAX_PICTURES)
        return 2;
    // (exactly as large as the data; the state is of 8-byte words, as the contract aligns it)
    std::vector<uint64_t> state((size_t)n * tracks_stride(max_tracks) / 8u);
    if (!read_all(in, state.data(), state.size() * 8u)) return 2;

    static TracksLds lds;
    static TracksLane threads[TRACKS_THREADS];
    auto each = [&](auto f) {
        for (int k = 0; k < (int)TRACKS_THREADS; k++) {
            const int t = order == 0 ? k : (order == 1 ? (int)TRACKS_THREADS - 1 - k : k * 101 % (int)TRACKS_THREADS);
            f(t, threads[t]);
        }
    };
    for (uint32_t c = 0; c < n_calls; c++) {
        uint32_t ch[4];
        if (!read_all(in, ch, sizeof ch)) return 2;
        const uint32_t n_rois = ch[0], has_cut = ch[1], cut_words = ch[2];
        if (n_rois > TRACKS_MAX_ROIS) return 2;
        std::vector<h263mi_roi> rois(n_rois);
        std::vector<h263mi_region_info> info_in(n);
        std::vector<uint32_t> cut(cut_words), cut_count(has_cut ? 1 : 0);
        if (!read_all(in, rois.data(), rois.size() * sizeof(h263mi_roi)) ||
            !read_all(in, info_in.data(), info_in.size() * sizeof(h263mi_region_info)) || !read_all(in, cut.data(), 4 * cut.size()))
            return 2;
        if (has_cut) cut_count[0] = ch[3];
        std::vector<h263mi_roi> table(max_out);
        std::vector<h263mi_track_ref> refs(flags & 1u ? max_out : 0u);
        std::vector<h263mi_track_info> info(n);
        std::vector<uint32_t> count(2);
        memset(table.data(), 0xC3, table.size() * sizeof(h263mi_roi));
        if (!refs.empty()) memset(refs.data(), 0xC3, refs.size() * sizeof(h263mi_track_ref));
        if (!info.empty()) memset(info.data(), 0xC3, info.size() * sizeof(h263mi_track_info));
        memset(count.data(), 0xC3, 8);

        TracksArgs a{};
        a.rois = rois.empty() ? nullptr : rois.data();
        a.info_in = info_in.data();
        a.state = reinterpret_cast<uint8_t *>(state.data());
        a.cut = has_cut ? cut.data() : nullptr;
        a.cut_count = has_cut ? cut_count.data() : nullptr;
        a.info = info.data();
        a.n_rois = n_rois, a.n_pictures = n, a.w = w, a.h = h;
        a.max_tracks = max_tracks, a.iou_permille = hd[4], a.max_missed = hd[5], a.min_hits = hd[6], a.emit_period = hd[7];
        for (uint32_t p = 0; p < n; p++) {                     // blockIdx.x = picture
            memset(&lds, 0xA5, sizeof lds);
            memset(threads, 0x5A, sizeof threads);
            tracks_picture(a, lds, p, each);
        }
        const TracksPackArgs f{a.state, table.data(), refs.empty() ? nullptr : refs.data(), info.data(), count.data(), n, max_tracks, max_out, 0};
        static TracksPackLds plds;
        static TracksPackLane lanes[64];
        memset(&plds, 0xA5, sizeof plds);
        memset(lanes, 0x5A, sizeof lanes);
        tracks_pack(f, plds, [&](auto g) {
            for (int l = 0; l < 64; l++) g(l, lanes[l]);
        });
        if (!write_all(out, state.data(), state.size() * 8u) || !write_all(out, table.data(), table.size() * sizeof(h263mi_roi)) ||
            !write_all(out, refs.data(), refs.size() * sizeof(h263mi_track_ref)) ||
            !write_all(out, info.data(), info.size() * sizeof(h263mi_track_info)) || !write_all(out, count.data(), 8))
            return 2;
    }
    fclose(in);
    fclose(out);
    return 0;
}
