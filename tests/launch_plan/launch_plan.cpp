// launch_plan.cpp -- the launch plans of the banded kernels and of k_change on the CPU (TEST INFRASTRUCTURE).
//
// The plans (resize_plan ... roi_plan beside their Args in h263-rs_amd/csrc/*.inl, change_plan in change_kernel.inl) are all that
// decides which waves a launch has and which arguments it refuses.  Built by tests/test_launch_plan.py with
// g++ -fsanitize=address,undefined into a temporary directory; never part of the product.
//
//   launch_plan <cases> <out>
//   cases: one case a line: the plan's name, then field=value pairs laid over an argument set that the plan accepts (below);
//          null=<pointer> clears a pointer
//   out  : a line a case: "refused", or for a banded plan "ok bands chunk segs_y x y z" (segs_y 0 where the kernel has none), for
//          change "ok items_per_wave waves pictures p0,p0,..." -- the first picture of every launch of launch_change's loop
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>

#include "../../h263-rs_amd/csrc/change_kernel.inl"
#include "../../h263-rs_amd/csrc/plane_filter_kernel.inl"
#include "../../h263-rs_amd/csrc/roi_kernel.inl"

using namespace h263mi;

typedef std::map<std::string, std::string> Fields;

static uint8_t some[64];                                 // what every pointer of an accepted set points at: no plan reads through one

template <class T>
static T *ptr(const Fields &f, const char *name)
{
    auto it = f.find("null");
    return it != f.end() && it->second == name ? nullptr : reinterpret_cast<T *>(some);
}

static uint32_t num(const Fields &f, const char *name, uint32_t otherwise)
{
    auto it = f.find(name);
    return it == f.end() ? otherwise : (uint32_t)strtoul(it->second.c_str(), nullptr, 10);
}

static void banded(FILE *out, bool ok, const LaunchDims &d, uint32_t bands, uint32_t chunk, uint32_t segs_y)
{
    if (ok) fprintf(out, "ok %u %u %u %u %u %u\n", bands, chunk, segs_y, d.x, d.y, d.z);
    else fprintf(out, "refused\n");
}

// 320 x 240 pictures, three of them, into 100 x 50
static ResizeArgs resize_args(const Fields &f)
{
    ResizeArgs r{};
    r.src = ptr<const uint8_t>(f, "src");
    r.w = num(f, "w", 320), r.h = num(f, "h", 240), r.ow = num(f, "ow", 100), r.oh = num(f, "oh", 50);
    r.n_pictures = num(f, "n", 3);
    return r;
}

static TensorArgs tensor_args(const Fields &f)
{
    TensorArgs t{};
    t.r = resize_args(f);
    t.dtype = num(f, "dtype", TENSOR_BF16);
    return t;
}

// a 90 x 45 rectangle at (10, 5) of a 100 x 50 output: it touches the right and the bottom edge
static FrameRect rect(const Fields &f)
{
    FrameRect r{};
    r.cw = num(f, "cw", 100), r.ch = num(f, "ch", 50), r.dx = num(f, "dx", 10), r.dy = num(f, "dy", 5), r.keep = num(f, "keep", 1);
    return r;
}

static FilterAxis axis(const Fields &f, const std::string &name)
{
    return FilterAxis{ptr<const FilterSpan>(f, (name + ".span").c_str()), ptr<const int32_t>(f, (name + ".coeff").c_str()),
                      num(f, (name + ".ksize").c_str(), 4)};
}

static FilterArgs filter_args(const Fields &f)
{
    FilterArgs a{};
    a.src = ptr<const uint8_t>(f, "src");
    a.dst = ptr<uint8_t *const>(f, "dst");
    a.x = axis(f, "x"), a.y = axis(f, "y");
    a.w = num(f, "w", 320), a.h = num(f, "h", 240), a.dw = num(f, "dw", 90), a.dh = num(f, "dh", 45);
    a.n_pictures = num(f, "n", 3);
    a.f = rect(f);
    return a;
}

static void run_case(FILE *out, const std::string &plan, const Fields &f)
{
    LaunchDims d{};
    if (plan == "resize") {
        ResizeArgs a = resize_args(f);
        const bool ok = resize_plan(a, d);
        banded(out, ok, d, a.bands, a.chunk, 0);
    } else if (plan == "tensor") {
        TensorArgs a = tensor_args(f);
        const bool ok = tensor_resize_plan(a, d);
        banded(out, ok, d, a.r.bands, a.r.chunk, 0);
    } else if (plan == "framed" || plan == "framed_tensor") {
        FramedTensorArgs a{};
        a.t = tensor_args(f);
        a.t.r.ow = num(f, "dw", 90), a.t.r.oh = num(f, "dh", 45);
        a.f = rect(f);
        FramedResizeArgs ra{a.t.r, a.f};
        const bool ok = plan == "framed" ? framed_resize_plan(ra, d) : framed_tensor_plan(a, d);
        const ResizeArgs &r = plan == "framed" ? ra.r : a.t.r;
        banded(out, ok, d, r.bands, r.chunk, 0);
    } else if (plan == "filter" || plan == "filter_tensor") {
        TensorFilterArgs a{};
        a.fl = filter_args(f);
        a.t.dtype = num(f, "dtype", TENSOR_BF16);
        const bool ok = plan == "filter" ? filter_rgba_plan(a.fl, d) : filter_tensor_plan(a, d);
        banded(out, ok, d, a.fl.bands, a.fl.chunk, 0);
    } else if (plan == "plane_resize") {
        PlaneResizeArgs a{};
        a.ow = num(f, "ow", 100), a.oh = num(f, "oh", 50), a.cow = num(f, "cow", 50), a.coh = num(f, "coh", 25);
        a.n_pictures = num(f, "n", 3);
        const bool ok = plane_resize_plan(a, d);
        banded(out, ok, d, a.bands, a.chunk, a.segs_y);
    } else if (plan == "plane_filter") {
        PlaneFilterArgs a{};
        a.src = ptr<const uint8_t>(f, "src");
        a.dst = ptr<const PlaneDst>(f, "dst");
        a.xy = axis(f, "xy"), a.yy = axis(f, "yy"), a.xc = axis(f, "xc"), a.yc = axis(f, "yc");
        a.w = num(f, "w", 321), a.h = num(f, "h", 241), a.cw = num(f, "cw", 161), a.ch = num(f, "ch", 121);
        a.ow = num(f, "ow", 100), a.oh = num(f, "oh", 50), a.cow = num(f, "cow", 50), a.coh = num(f, "coh", 25);
        a.n_pictures = num(f, "n", 3);
        const bool ok = plane_filter_plan(a, d);
        banded(out, ok, d, a.bands, a.chunk, a.segs_y);
    } else if (plan == "roi") {
        RoiArgs a{};
        a.t = tensor_args(f);
        a.rois = ptr<const RoiRecord>(f, "rois");
        a.dst = ptr<uint8_t>(f, "dst");
        a.n_rois = num(f, "n_rois", 5);
        const bool ok = roi_plan(a, d);
        banded(out, ok, d, a.t.r.bands, a.t.r.chunk, 0);
    } else if (plan == "change") {
        // 64 pictures of 1920 x 1080 in cells of 16 x 16
        ChangeArgs a{};
        a.cur = ptr<const uint8_t>(f, "cur");
        a.prev = ptr<uint8_t>(f, "prev");
        a.summary = ptr<h263mi_change_summary>(f, "summary");
        a.w = num(f, "w", 1920), a.h = num(f, "h", 1080), a.gw = num(f, "gw", 120), a.gh = num(f, "gh", 68);
        a.cell_log2 = num(f, "cell_log2", 4), a.segs = num(f, "segs", 2), a.n_pictures = num(f, "n", 64);
        ChangeLaunch l{};
        if (!change_plan(a, l, num(f, "items_per_wave", 0))) {
            fprintf(out, "refused\n");
            return;
        }
        fprintf(out, "ok %u %u %u ", a.items_per_wave, l.waves, l.pictures);
        for (uint32_t p0 = 0; p0 < a.n_pictures; p0 += l.pictures) fprintf(out, p0 ? ",%u" : "%u", p0);      // (launch_change's loop)
        fprintf(out, "\n");
    } else {
        fprintf(out, "unknown plan\n");
    }
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "r"), *out = fopen(argv[2], "w");
    if (!in || !out) return 2;
    char line[1024];
    while (fgets(line, sizeof line, in)) {
        std::string plan;
        Fields f;
        for (char *tok = strtok(line, " \n"); tok; tok = strtok(nullptr, " \n")) {
            char *eq = strchr(tok, '=');
            if (!eq) plan = tok;
            else f[std::string(tok, eq)] = eq + 1;
        }
        if (!plan.empty()) run_case(out, plan, f);
    }
    fclose(in);
    return fclose(out) ? 2 : 0;
}
