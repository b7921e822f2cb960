// hist_plan.cpp -- the launch plan of k_hist on the CPU (TEST INFRASTRUCTURE).
//
// hist_plan (beside HistArgs in h263-rs_amd/csrc/hist_kernel.inl) is all that decides which waves a launch of k_hist has, how many
// work items each takes, how a call is split into launches and which arguments the launcher refuses.  Built by
// tests/test_hist_plan.py with g++ -fsanitize=address,undefined into a temporary directory; never part of the product.
//
//   hist_plan <cases> <out>
//   cases: one case a line: field=value pairs laid over an argument set that the plan accepts (64 pictures of 1920 x 1080);
//          null=<pointer> clears a pointer; a line may be empty
//   out  : a line a case: "refused", or "ok items_per_wave waves pictures p0,p0,..." -- the first picture of every launch of
//          launch_hist's loop
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>

#include "../../h263-rs_amd/csrc/hist_kernel.inl"

using namespace h263mi;

typedef std::map<std::string, std::string> Fields;

static uint8_t some[64];                                 // what every pointer of the accepted set points at: the plan reads through none

static uint32_t num(const Fields &f, const char *name, uint32_t dflt)
{
    const auto it = f.find(name);
    return it == f.end() ? dflt : (uint32_t)strtoul(it->second.c_str(), nullptr, 10);
}

static void run_case(const Fields &f, FILE *out)
{
    const auto null = f.find("null");
    HistArgs a{};
    a.src = null != f.end() && null->second == "src" ? nullptr : some;
    a.hist = null != f.end() && null->second == "hist" ? nullptr : reinterpret_cast<uint32_t *>(some);
    a.w = num(f, "w", 1920), a.h = num(f, "h", 1080), a.n_pictures = num(f, "n", 64);
    a.align = num(f, "align", 16), a.segs = num(f, "segs", 2), a.bands = num(f, "bands", 135);
    HistLaunch l{};
    if (!hist_plan(a, l, num(f, "items_per_wave", 0))) {
        fprintf(out, "refused\n");
        return;
    }
    fprintf(out, "ok %u %u %u ", a.items_per_wave, l.waves, l.pictures);
    for (uint32_t p0 = 0; p0 < a.n_pictures; p0 += l.pictures) fprintf(out, p0 ? ",%u" : "%u", p0);          // (launch_hist's loop)
    fprintf(out, "\n");
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
