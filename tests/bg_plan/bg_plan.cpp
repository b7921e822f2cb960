// bg_plan.cpp -- the launch plan of k_bg on the CPU (TEST INFRASTRUCTURE).
//
// bg_plan (beside BgArgs in h263-rs_amd/csrc/background_kernel.inl) is all that decides which waves a launch of k_bg has, how many
// work items each takes, how a call is split into launches and which arguments the launcher refuses.  This program lays a plan out
// as launch_background does -- launches of whole pictures from p0 on, blockIdx.y = picture, blockIdx.x = the wave -- walks every
// wave's items as bg_wave does (item first + i while i < items_per_wave and the cell row exists; item = cell row * segs + segment)
// and counts how often every (picture, cell row, segment) is taken.  Built by tests/test_bg_plan.py with
// g++ -fsanitize=address,undefined into a temporary directory; never part of the product.
//
//   bg_plan <cases> <out>
//   cases: one case a line: field=value pairs laid over an argument set that the plan accepts (64 pictures of 1920 x 1080, cells of
//          16); null=<pointer> clears a pointer
//   out  : a line a case: "refused", or "ok items_per_wave waves pictures launches largest_grid once" -- once = 1 when every work
//          item of the call is taken exactly once and no wave takes one that does not exist
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "../../h263-rs_amd/csrc/background_kernel.inl"

using namespace h263mi;

typedef std::map<std::string, std::string> Fields;

alignas(32) static uint8_t some[64];                     // what every pointer of the accepted set points at: the plan reads through none

static uint32_t num(const Fields &f, const char *name, uint32_t dflt)
{
    const auto it = f.find(name);
    return it == f.end() ? dflt : (uint32_t)strtoul(it->second.c_str(), nullptr, 10);
}

static void run_case(const Fields &f, FILE *out)
{
    const auto null = f.find("null");
    const std::string none = null == f.end() ? "" : null->second;
    BgArgs a{};
    a.cur = none == "cur" ? nullptr : some;
    a.state = none == "state" ? nullptr : some + num(f, "state_offset", 0);
    a.summary = none == "summary" ? nullptr : reinterpret_cast<h263mi_change_summary *>(some);
    a.cut = none == "cut" ? nullptr : reinterpret_cast<const uint32_t *>(some);
    a.cut_count = none == "cut_count" ? nullptr : reinterpret_cast<const uint32_t *>(some);
    a.w = num(f, "w", 1920), a.h = num(f, "h", 1080), a.n_pictures = num(f, "n", 64);
    a.cell_log2 = num(f, "cl", 4);
    const uint32_t c = a.cell_log2 < 32 ? 1u << a.cell_log2 : 1u;
    a.gw = num(f, "gw", a.w ? (a.w + c - 1) / c : 0), a.gh = num(f, "gh", a.h ? (a.h + c - 1) / c : 0);
    a.segs = num(f, "segs", (a.w + CHANGE_SEG - 1) / CHANGE_SEG);
    a.bpitch = num(f, "bpitch", bg_pitch(a.w));
    a.state_stride = (uint64_t)BG_HEAD_BYTES + (uint64_t)a.h * bg_pitch(a.w) + num(f, "stride_plus", 0);
    a.learn_shift = num(f, "learn", 4), a.fg_learn_shift = num(f, "fg_learn", 255), a.pixel_threshold = num(f, "pix_thr", 24);
    BgLaunch l{};
    if (!bg_plan(a, l, num(f, "items_per_wave", 0))) {
        fprintf(out, "refused\n");
        return;
    }
    const uint32_t items = a.gh * a.segs;
    std::vector<uint8_t> taken((size_t)a.n_pictures * items, 0);
    bool once = l.pictures >= 1;
    uint64_t launches = 0, largest = 0;
    for (uint32_t p0 = 0; once && p0 < a.n_pictures; p0 += l.pictures) {                // (launch_background's loop)
        const uint32_t n = a.n_pictures - p0 < l.pictures ? a.n_pictures - p0 : l.pictures;
        launches++;
        if ((uint64_t)l.waves * n > largest) largest = (uint64_t)l.waves * n;
        for (uint32_t y = 0; y < n; y++)
            for (uint32_t x = 0; x < l.waves; x++) {
                const uint32_t first = x * a.items_per_wave;                            // (bg_wave's walk)
                uint32_t cy = first / a.segs, seg = first - cy * a.segs, took = 0;
                for (uint32_t i = 0; i < a.items_per_wave && cy < a.gh; i++) {
                    uint8_t &t = taken[(size_t)(p0 + y) * items + (size_t)cy * a.segs + seg];
                    once &= t == 0;
                    t = 1;
                    took++;
                    if (++seg == a.segs) seg = 0, cy++;
                }
                once &= took >= 1;                                                      // (no wave without work)
            }
    }
    for (uint8_t t : taken) once &= t == 1;
    fprintf(out, "ok %u %u %u %llu %llu %d\n", a.items_per_wave, l.waves, l.pictures, (unsigned long long)launches,
            (unsigned long long)largest, once ? 1 : 0);
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "r"), *out = fopen(argv[2], "w");
    if (!in || !out) return 2;
    char line[1024];
    while (fgets(line, sizeof line, in)) {
        Fields f;
        for (char *tok = strtok(line, " \n"); tok; tok = strtok(nullptr, " \n")) {
            char *eq = strchr(tok, '=');
            if (!eq) return 2;
            f[std::string(tok, eq)] = std::string(eq + 1);
        }
        run_case(f, out);
    }
    fclose(in);
    fclose(out);
    return 0;
}
