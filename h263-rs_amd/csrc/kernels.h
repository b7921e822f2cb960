// kernels.h -- host-visible launchers of the gfx950 kernels (decode_kernels.hip, output_kernels.hip,
// analysis_kernels.hip, support_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "dev_common.h"
#include "background_kernel.inl"
#include "change_kernel.inl"
#include "digest_kernel.inl"
#include "filter_kernel.inl"
#include "hist_kernel.inl"
#include "plane_filter_kernel.inl"
#include "plane_resize_kernel.inl"
#include "regions_kernel.inl"
#include "resize_kernel.inl"
#include "roi_kernel.inl"
#include "tensor_resize_kernel.inl"
#include "tracks_kernel.inl"

namespace h263mi {

struct SynthArgs {
    int kind;
    uint32_t n_streams, first_stream_id, frame_idx, mbs_per_picture;
    uint32_t stream_stride;     // picture p is stream first_stream_id + p * stream_stride (1: consecutive ids)
    MbRecord *mbs;              // device, n_streams * mbs_per_picture
    uint32_t *counts;           // device scratch, one per macroblock
    uint32_t *totals;           // device, coded blocks per picture
    int16_t *coeffs;            // device pool
    const uint64_t *coeff_base; // device, per picture
};

// geometry of the merged launch (k_frame), made by its launcher
struct FrameGeom {
    uint32_t groups;            // groups of 32 luma rows per picture
    uint32_t recon_per_group;   // reconstruction waves per group: 2 per 8x2-macroblock tile (one per macroblock row)
    uint32_t post_per_group;    // post tiles (waves) per group
    uint32_t inv_per_group;     // ceil(2^32 / (recon_per_group + post_per_group))
    uint32_t flip;              // walk the pictures of the batch in descending order
    uint32_t bands;             // XCDs that share one picture (8, 4 or 2): 8 / bands pictures side by side
};
// `words` (HOST pointer, n_pictures STREAM_* words, or nullptr): the streams of the launch differ -- each picture's waves read
// its word.  Up to STREAM_WORDS_INLINE pictures they travel in the kernel arguments; beyond that the caller has put them into
// device memory (args.stream_state) and passes nullptr here.
hipError_t launch_recon(const ReconArgs &args, hipStream_t stream, const uint32_t *words = nullptr);
// k_recon over `rargs` and k_post over `pargs` (same number of pictures, same picture size) as ONE launch.
// `descending`: walk the pictures last to first.  A caller that alternates the direction from one frame index to the
// next reads the planes it wrote last -- the ones still in the infinity cache -- first (2 % on a 64-stream batch).
hipError_t launch_frame(const ReconArgs &rargs, const PostArgs &pargs, hipStream_t stream, bool descending, const uint32_t *words = nullptr);
hipError_t launch_post(const PostArgs &args, hipStream_t stream, const uint32_t *words = nullptr);
// The YUV instantiations (k_post_yuv, k_frame_yuv): the post-processing writes the filtered planes to args.planes_out in the
// shape `yuv` (h263mi_yuv_layout) and no RGBA.  Declared weak for the same reason as launch_rgba_resize below; the batch
// refuses to render planes in a layout without them.
hipError_t launch_post_yuv(const PostArgs &args, const YuvOut &yuv, hipStream_t stream, const uint32_t *words = nullptr) __attribute__((weak));
hipError_t launch_frame_yuv(const ReconArgs &rargs, const PostArgs &pargs, const YuvOut &yuv, hipStream_t stream, bool descending,
                            const uint32_t *words = nullptr) __attribute__((weak));
// k_rgba_resize over args.n_pictures pictures (resize_kernel.inl; bands and chunk are set here).  Declared weak: the host
// objects are also linked, in the CPU suite's ThreadSanitizer build (tests/tsan), against a stub runtime that has no resize
// launcher.  The library always defines it (output_kernels.hip); h263mi_batch::launch_resize refuses to run without it.
hipError_t launch_rgba_resize(const ResizeArgs &args, hipStream_t stream) __attribute__((weak));
// k_tensor_resize over args.r.n_pictures pictures (tensor_resize_kernel.inl; bands and chunk are set here): k_rgba_resize's launch
// shape, planar float stores.  Weak like launch_rgba_resize; h263mi_batch::launch_resize refuses to write a tensor without it.
hipError_t launch_tensor_resize(const TensorArgs &args, hipStream_t stream) __attribute__((weak));
// k_rgba_resize_framed / k_tensor_resize_framed (h263mi_framing): args.r describes the resize inside the destination rectangle,
// args.f the W' x H' output around it, which is what the launch covers (bands and chunk are set here).  Weak like
// launch_rgba_resize; the host refuses a framed shape without them.
hipError_t launch_rgba_resize_framed(const FramedResizeArgs &args, hipStream_t stream) __attribute__((weak));
hipError_t launch_tensor_resize_framed(const FramedTensorArgs &args, hipStream_t stream) __attribute__((weak));
// k_roi_tensor over args.n_rois regions of interest (roi_kernel.inl; bands and chunk are set here): k_tensor_resize's launch shape with
// the region in the place of the picture.  Weak like launch_rgba_resize; h263mi_roi_tensor_on refuses to run without it.
hipError_t launch_roi_tensor(const RoiArgs &args, hipStream_t stream) __attribute__((weak));
// k_change over the args.n_pictures x gh x segs work items of a change map (change_kernel.inl; p0 and items_per_wave are set here: a call of very many
// items goes out in several launches), then, with sel, k_change_select over the summaries.  The caller has cleared the summaries
// on the stream.  Weak like launch_rgba_resize; the change-map entry points refuse to run without it.
hipError_t launch_change(const ChangeArgs &args, const ChangeSelectArgs *sel, hipStream_t stream) __attribute__((weak));
// k_rgba_filter / k_tensor_filter (h263mi_filter: bilinear, bicubic; filter_kernel.inl): args.f is the W' x H' output that the
// launch covers and the place of the args.dw x args.dh rectangle in it (bands and chunk are set here).  Weak like
// launch_rgba_resize; the host refuses a filtered shape without them.
hipError_t launch_rgba_filter(const FilterArgs &args, hipStream_t stream) __attribute__((weak));
hipError_t launch_tensor_filter(const TensorFilterArgs &args, hipStream_t stream) __attribute__((weak));
// k_plane_resize over args.n_pictures pictures (plane_resize_kernel.inl; bands, chunk and segs_y are set here): the luma and
// chroma planes of every picture in ONE launch.  Weak like launch_rgba_resize; h263mi_batch::launch_plane_resize refuses to run
// without it.
hipError_t launch_plane_resize(const PlaneResizeArgs &args, hipStream_t stream) __attribute__((weak));
// k_plane_filter over args.n_pictures pictures (plane_filter_kernel.inl; bands, chunk and segs_y are set here): k_plane_resize's
// launch shape, Pillow's bilinear / bicubic taps in the place of the area average.  Weak like launch_rgba_resize; the host
// refuses a filtered YUV shape without it.
hipError_t launch_plane_filter(const PlaneFilterArgs &args, hipStream_t stream) __attribute__((weak));
// k_digest over args.n_items work items, then k_digest_final over fin.n_digests digests (digest_kernel.inl): the launch pair of one
// digest call, whatever it covers.  Weak like launch_rgba_resize; the digest entry points refuse to run without it.
hipError_t launch_digest(const DigestArgs &args, const DigestFinalArgs &fin, hipStream_t stream) __attribute__((weak));
// k_hist over the args.n_pictures x bands x segs work items of a histogram call (hist_kernel.inl; p0 and items_per_wave are set
// here: a call of very many items goes out in several launches of whole pictures), then k_hist_final over the pictures and, with
// sel, k_hist_select over the statistics.  The caller has cleared the histograms on the stream.  Weak like launch_rgba_resize; the
// histogram entry points refuse to run without it.
hipError_t launch_hist(const HistArgs &args, const HistFinalArgs &fin, const HistSelectArgs *sel, hipStream_t stream) __attribute__((weak));
// k_regions, one workgroup per picture of args.n_pictures grids (regions_kernel.inl), then k_regions_pack, one wave, over the
// pictures' staged entries: the launch pair of one regions call; without pictures the pack alone, which still fills the table.
// Weak like launch_rgba_resize; the regions entry points refuse to run without it.
hipError_t launch_regions(const RegionsArgs &args, const RegionsPackArgs &pack, hipStream_t stream) __attribute__((weak));
// k_tracks, one workgroup per picture of args.n_pictures states (tracks_kernel.inl), then k_tracks_pack, one wave, over the
// pictures' emitted slots: the launch pair of one tracks call; without pictures the pack alone, which still fills the table.
// Weak like launch_rgba_resize; the tracks entry points refuse to run without it.
hipError_t launch_tracks(const TracksArgs &args, const TracksPackArgs &pack, hipStream_t stream) __attribute__((weak));
// k_bg_begin over the pictures, k_bg over the args.n_pictures x gh x segs work items of a background call (background_kernel.inl; p0
// and items_per_wave are set here: bg_plan), then, with sel, k_change_select over the summaries.  k_bg_begin clears the summaries:
// the caller queues nothing in front.  Weak like launch_rgba_resize; the background entry points refuse to run without it.
hipError_t launch_background(const BgArgs &args, const ChangeSelectArgs *sel, hipStream_t stream) __attribute__((weak));
hipError_t launch_synth_headers(const SynthArgs &args, hipStream_t stream);
hipError_t launch_synth_coeffs(const SynthArgs &args, hipStream_t stream);
// streaming probes: mode 0 copy in -> out, 1 read in (out = 16-byte sink), 2 write out; bytes is a multiple of 16;
// shape < probe_shapes(mode) picks the launch shape (support_kernels.hip)
int probe_shapes(int mode);
const char *probe_shape_name(int mode, int shape);
hipError_t launch_probe(int mode, int shape, const void *in, void *out, size_t bytes, hipStream_t stream);

}  // namespace h263mi
