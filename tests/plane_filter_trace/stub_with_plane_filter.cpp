// stub_with_plane_filter.cpp -- the stub runtime of tests/tsan with the one launcher it lacks: launch_plane_filter
// (TEST INFRASTRUCTURE).  stub_runtime.cpp is included as it stands, so that this launcher describes its launch through the same
// recorder, in the same ` key=value` form as launch_plane_resize there.
#include "../tsan/stub_runtime.cpp"

namespace h263mi {

// the four tap tables as they lie behind a.xy.span (plane_filter_kernel.inl: plane_filter_axes): where, 32-bit words, FNV-1a
static void put_tables(std::string &s, const PlaneFilterArgs &a)
{
    const uint64_t words = 2ull * (a.ow + a.oh + a.cow + a.coh) + (uint64_t)a.ow * a.xy.ksize + (uint64_t)a.oh * a.yy.ksize +
                           (uint64_t)a.cow * a.xc.ksize + (uint64_t)a.coh * a.yc.ksize;
    uint64_t h = 0xcbf29ce484222325ull;
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(a.xy.span);
    for (size_t i = 0; i < (size_t)words * 4; i++) h = (h ^ bytes[i]) * 0x100000001b3ull;
    appendf(s, " tables=%s#%llu:%016llx", where(a.xy.span).c_str(), (unsigned long long)words, (unsigned long long)h);
    // the axes must be the ones of that block, in its order
    const bool in_order = (const void *)a.yy.span == (const void *)(a.xy.span + a.ow) && (const void *)a.xy.coeff == (const void *)(a.yy.span + a.oh) &&
                          a.yy.coeff == a.xy.coeff + (size_t)a.ow * a.xy.ksize &&
                          (const void *)a.xc.span == (const void *)(a.yy.coeff + (size_t)a.oh * a.yy.ksize) &&
                          (const void *)a.yc.span == (const void *)(a.xc.span + a.cow) && (const void *)a.xc.coeff == (const void *)(a.yc.span + a.coh) &&
                          a.yc.coeff == a.xc.coeff + (size_t)a.cow * a.xc.ksize;
    put(s, "axes_in_order", in_order ? 1u : 0u);
}

hipError_t launch_plane_filter(const PlaneFilterArgs &a, hipStream_t on)
{
    std::string s = "plane_filter " + stream_name(on);
    put(s, "n", a.n_pictures);
    put_ptr(s, "src", a.src);
    put(s, "w", a.w), put(s, "h", a.h), put(s, "cw", a.cw), put(s, "ch", a.ch);
    put(s, "ow", a.ow), put(s, "oh", a.oh), put(s, "cow", a.cow), put(s, "coh", a.coh);
    put(s, "pitch_y", a.pitch_y), put(s, "pitch_c", a.pitch_c);
    put(s, "nv12", a.nv12), put(s, "wide", a.wide);
    put(s, "d_y", a.d_y), put(s, "d_c", a.d_c);
    put(s, "ksx_y", a.xy.ksize), put(s, "ksy_y", a.yy.ksize), put(s, "ksx_c", a.xc.ksize), put(s, "ksy_c", a.yc.ksize);
    put_tables(s, a);
    put_array(s, "dst", a.dst, a.n_pictures,
              [](const PlaneDst &d) { return "(" + where(d.p[0]) + " " + where(d.p[1]) + " " + where(d.p[2]) + ")"; });
    emit(s);
    return hipSuccess;
}

}  // namespace h263mi
