// analysis_kernels.hip -- digests, change maps, histograms, motion regions, region tracks and background models of pictures in device memory: __global__ wrappers and launchers.
// Built with the flags of decode_kernels.hip.
#include "kernels.h"

#include "background_kernel.inl"
#include "change_kernel.inl"
#include "digest_kernel.inl"
#include "hist_kernel.inl"
#include "regions_kernel.inl"
#include "tracks_kernel.inl"

namespace h263mi {

// ---------------------------------------------------------------------------------------
// k_digest, k_digest_final: Adler-32 of pitched rows in device memory (digest_kernel.inl).  One wave per workgroup, no barrier;
// a wave takes the work items blockIdx.x, blockIdx.x + gridDim.x, ... -- one each unless a call has more items than
// DIGEST_GRID_MAX -- and adds their terms to the digests' accumulators; the second launch reduces and packs them.
// ---------------------------------------------------------------------------------------
constexpr uint64_t DIGEST_GRID_MAX = 1u << 20;

__global__ __launch_bounds__(64) void k_digest(DigestArgs a)
{
    __shared__ __attribute__((aligned(16))) DigestLds lds;
    const int lane = threadIdx.x & 63;
    DigestLane t;
    for (uint64_t item = blockIdx.x; item < a.n_items; item += gridDim.x)
        digest_item(a, lds, item, [&](auto f) { f(lane, t); });
}

__global__ __launch_bounds__(256) void k_digest_final(DigestFinalArgs f)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < f.n_digests) digest_final(f, k);
}

hipError_t launch_digest(const DigestArgs &args, const DigestFinalArgs &fin, hipStream_t stream)
{
    if (!fin.n_digests) return hipSuccess;
    if (args.n_items) {
        const uint32_t grid = (uint32_t)(args.n_items < DIGEST_GRID_MAX ? args.n_items : DIGEST_GRID_MAX);
        hipLaunchKernelGGL(k_digest, dim3(grid), dim3(64), 0, stream, args);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_digest_final, dim3((fin.n_digests + 255u) / 256u), dim3(256), 0, stream, fin);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// k_change, k_change_select: change maps of 8-bit planes (h263mi_change_map_on, h263mi_batch_change_last; change_kernel.inl).
// One wave per workgroup, no barrier: blockIdx.x = the wave's run of items_per_wave work items (segments of CHANGE_SEG columns of
// a cell row, row after row), blockIdx.y = picture (from args.p0).  A launch holds at most CHANGE_GRID_MAX workgroups, whole
// pictures; the select kernel is one wave.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_change(ChangeArgs a)
{
    __shared__ __attribute__((aligned(16))) ChangeLds lds;
    const int lane = threadIdx.x & 63;
    ChangeLane t;
    change_wave(a, lds, a.p0 + blockIdx.y, blockIdx.x * a.items_per_wave, [&](auto f) { f(lane, t); });
}

__global__ __launch_bounds__(64) void k_change_select(ChangeSelectArgs f)
{
    __shared__ __attribute__((aligned(16))) ChangeLds lds;
    const int lane = threadIdx.x & 63;
    ChangeLane t;
    change_select(f, lds, [&](auto g) { g(lane, t); });
}

hipError_t launch_change(const ChangeArgs &args, const ChangeSelectArgs *sel, hipStream_t stream)
{
    if (args.n_pictures) {
        ChangeArgs a = args;
        ChangeLaunch l;
        if (!change_plan(a, l)) return hipErrorInvalidValue;
        for (a.p0 = 0; a.p0 < a.n_pictures; a.p0 += l.pictures) {
            const uint32_t n = a.n_pictures - a.p0 < l.pictures ? a.n_pictures - a.p0 : l.pictures;
            hipLaunchKernelGGL(k_change, dim3(l.waves, n), dim3(64), 0, stream, a);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
    }
    if (sel) {
        if (!sel->selected || !sel->count || (sel->n_pictures && !sel->summary)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_change_select, dim3(1), dim3(64), 0, stream, *sel);
        return hipGetLastError();
    }
    return hipSuccess;
}

// ---------------------------------------------------------------------------------------
// k_hist, k_hist_final, k_hist_select: histograms of 8-bit planes, their statistics and the scene-cut list (h263mi_hist_on,
// h263mi_batch_hist_last; hist_kernel.inl).  One wave per workgroup, no barrier.  k_hist: blockIdx.x = the wave's run of
// items_per_wave work items (segments of HIST_SEG columns of a band of HIST_ROWS rows, band after band), blockIdx.y = picture (from
// args.p0); a launch holds at most HIST_GRID_MAX workgroups, whole pictures.  k_hist_final: blockIdx.x = picture.  The select
// kernel is one wave.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_hist(HistArgs a)
{
    __shared__ __attribute__((aligned(16))) HistLds lds;
    const int lane = threadIdx.x & 63;
    HistLane t;
    hist_wave(a, lds, a.p0 + blockIdx.y, blockIdx.x * a.items_per_wave, [&](auto f) { f(lane, t); });
}

__global__ __launch_bounds__(64) void k_hist_final(HistFinalArgs f)
{
    __shared__ __attribute__((aligned(16))) HistFinalLds lds;
    const int lane = threadIdx.x & 63;
    HistLane t;
    hist_final(f, lds, blockIdx.x, [&](auto g) { g(lane, t); });
}

__global__ __launch_bounds__(64) void k_hist_select(HistSelectArgs f)
{
    __shared__ __attribute__((aligned(16))) HistFinalLds lds;
    const int lane = threadIdx.x & 63;
    HistLane t;
    hist_select(f, lds, [&](auto g) { g(lane, t); });
}

hipError_t launch_hist(const HistArgs &args, const HistFinalArgs &fin, const HistSelectArgs *sel, hipStream_t stream)
{
    if (args.n_pictures) {
        HistArgs a = args;
        HistLaunch l;
        if (!hist_plan(a, l) || fin.n_pictures != a.n_pictures || !fin.hist || !fin.stats || (fin.roll && !fin.prev))
            return hipErrorInvalidValue;
        for (a.p0 = 0; a.p0 < a.n_pictures; a.p0 += l.pictures) {
            const uint32_t n = a.n_pictures - a.p0 < l.pictures ? a.n_pictures - a.p0 : l.pictures;
            hipLaunchKernelGGL(k_hist, dim3(l.waves, n), dim3(64), 0, stream, a);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(k_hist_final, dim3(fin.n_pictures), dim3(64), 0, stream, fin);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (sel) {
        if (!sel->selected || !sel->count || (sel->n_pictures && !sel->stats)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_hist_select, dim3(1), dim3(64), 0, stream, *sel);
        return hipGetLastError();
    }
    return hipSuccess;
}

// ---------------------------------------------------------------------------------------
// k_regions, k_regions_pack: the changed cells of a change map's grids as a table of ROI boxes (h263mi_regions_on,
// h263mi_batch_regions; regions_kernel.inl).  k_regions: blockIdx.x = picture, REGIONS_THREADS threads, the grid's parents and
// counts in sizeof(RegionsLds) bytes of static LDS -- one workgroup a CU.  The pack kernel is one wave.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(REGIONS_THREADS) void k_regions(RegionsArgs a)
{
    __shared__ __attribute__((aligned(16))) RegionsLds lds;
    const int tid = threadIdx.x;
    RegionsLane t;
    regions_picture(a, lds, blockIdx.x, [&](auto f) { f(tid, t); });
}

__global__ __launch_bounds__(64) void k_regions_pack(RegionsPackArgs f)
{
    __shared__ __attribute__((aligned(16))) RegionsPackLds lds;
    const int lane = threadIdx.x & 63;
    RegionsPackLane t;
    regions_pack(f, lds, [&](auto g) { g(lane, t); });
}

hipError_t launch_regions(const RegionsArgs &args, const RegionsPackArgs &pack, hipStream_t stream)
{
    if (!pack.rois || !pack.count || !pack.max_rois || pack.max_rois > REGIONS_MAX_ROIS || pack.n_pictures != args.n_pictures)
        return hipErrorInvalidValue;
    if (args.n_pictures) {
        if (!args.cells || !args.work || !args.info || pack.work != args.work || pack.info != args.info || !args.gw || !args.gh ||
            (uint64_t)args.gw * args.gh > REGIONS_MAX_CELLS || !args.max_per || args.max_per > REGIONS_MAX_PER_PICTURE ||
            pack.max_per != args.max_per || args.n_pictures > CHANGE_MAX_PICTURES)
            return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_regions, dim3(args.n_pictures), dim3(REGIONS_THREADS), 0, stream, args);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_regions_pack, dim3(1), dim3(64), 0, stream, pack);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// k_tracks, k_tracks_pack: the tracks of every picture, updated from a table of ROI boxes, and the table of the emitted tracks
// (h263mi_tracks_on, h263mi_batch_tracks; tracks_kernel.inl).  k_tracks: blockIdx.x = picture, TRACKS_THREADS threads,
// sizeof(TracksLds) bytes of static LDS.  The pack kernel is one wave.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(TRACKS_THREADS) void k_tracks(TracksArgs a)
{
    __shared__ __attribute__((aligned(16))) TracksLds lds;
    const int tid = threadIdx.x;
    TracksLane t;
    tracks_picture(a, lds, blockIdx.x, [&](auto f) { f(tid, t); });
}

__global__ __launch_bounds__(64) void k_tracks_pack(TracksPackArgs f)
{
    __shared__ __attribute__((aligned(16))) TracksPackLds lds;
    const int lane = threadIdx.x & 63;
    TracksPackLane t;
    tracks_pack(f, lds, [&](auto g) { g(lane, t); });
}

hipError_t launch_tracks(const TracksArgs &args, const TracksPackArgs &pack, hipStream_t stream)
{
    if (!pack.rois || !pack.count || !pack.max_out || pack.max_out > TRACKS_MAX_OUT || pack.n_pictures != args.n_pictures)
        return hipErrorInvalidValue;
    if (args.n_pictures) {
        if (!args.info_in || !args.state || !args.info || (args.n_rois && !args.rois) || args.n_rois > TRACKS_MAX_ROIS ||
            !args.cut != !args.cut_count || pack.state != args.state || pack.info != args.info || !args.max_tracks ||
            args.max_tracks > TRACKS_MAX || pack.max_tracks != args.max_tracks || args.n_pictures > TRACKS_MAX_PICTURES)
            return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_tracks, dim3(args.n_pictures), dim3(TRACKS_THREADS), 0, stream, args);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_tracks_pack, dim3(1), dim3(64), 0, stream, pack);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// k_bg_begin, k_bg: the background model of 8-bit planes (h263mi_background_on, h263mi_batch_background_last;
// background_kernel.inl).  k_bg_begin: one lane per picture.  k_bg: one wave per workgroup, no barrier, the grid of k_change --
// blockIdx.x = the wave's run of items_per_wave work items, blockIdx.y = picture (from args.p0); a launch holds at most BG_GRID_MAX
// workgroups, whole pictures.  The list is k_change_select's.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_bg_begin(BgArgs a)
{
    const uint32_t p = blockIdx.x * 64u + threadIdx.x;
    if (p < a.n_pictures) bg_begin(a, p);
}

__global__ __launch_bounds__(64) void k_bg(BgArgs a)
{
    __shared__ __attribute__((aligned(16))) ChangeLds lds;
    const int lane = threadIdx.x & 63;
    ChangeLane t;
    bg_wave(a, lds, a.p0 + blockIdx.y, blockIdx.x * a.items_per_wave, [&](auto f) { f(lane, t); });
}

hipError_t launch_background(const BgArgs &args, const ChangeSelectArgs *sel, hipStream_t stream)
{
    if (args.n_pictures) {
        BgArgs a = args;
        BgLaunch l;
        if (!bg_plan(a, l)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_bg_begin, dim3((a.n_pictures + 63u) / 64u), dim3(64), 0, stream, a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        for (a.p0 = 0; a.p0 < a.n_pictures; a.p0 += l.pictures) {
            const uint32_t n = a.n_pictures - a.p0 < l.pictures ? a.n_pictures - a.p0 : l.pictures;
            hipLaunchKernelGGL(k_bg, dim3(l.waves, n), dim3(64), 0, stream, a);
            e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
    }
    if (sel) {
        if (!sel->selected || !sel->count || (sel->n_pictures && !sel->summary)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_change_select, dim3(1), dim3(64), 0, stream, *sel);
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace h263mi
