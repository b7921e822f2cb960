// output_kernels.hip -- the banded output kernels: __global__ wrappers and launchers of the resizes, filters, planes and ROI
// tensors that read finished pictures.  Built with the flags of decode_kernels.hip.
#include "kernels.h"

#include "filter_kernel.inl"
#include "plane_filter_kernel.inl"
#include "plane_resize_kernel.inl"
#include "resize_kernel.inl"
#include "roi_kernel.inl"
#include "tensor_resize_kernel.inl"

namespace h263mi {

// ---------------------------------------------------------------------------------------
// k_rgba_resize: area-average resampling of full-size RGBA (resize_kernel.inl).  One wave per workgroup, no barrier;
// blockIdx.y = picture, blockIdx.z = segment of 64 output columns, blockIdx.x = band of RESIZE_ROWS output rows in XCD
// order: XCD k (blockIdx.x & 7, gridDim.x a multiple of 8) takes a contiguous run of bands, so the source rows that two
// neighbouring bands share are fetched into one L2.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_rgba_resize(ResizeArgs a)
{
    __shared__ __attribute__((aligned(16))) ResizeLds lds;
    const uint32_t band = xcd_band(blockIdx.x, a.chunk);
    if (band >= a.bands) return;
    const int lane = threadIdx.x & 63;
    ResizeLane t;
    resize_item(a, lds, band, blockIdx.z, blockIdx.y, [&](auto f) { f(lane, t); });
}

// A banded launch (band_launch.h) of `count` pictures or regions: none is no launch; the kernel's plan (beside its Args) refuses
// the arguments or fills bands, chunk (segs_y) and the grid; one wave per workgroup.
template <class Args>
static hipError_t launch_banded(void (*kernel)(Args), bool (*plan)(Args &, LaunchDims &), const Args &args, uint32_t count, hipStream_t stream)
{
    if (!count) return hipSuccess;
    Args a = args;
    LaunchDims d;
    if (!plan(a, d)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3(d.x, d.y, d.z), dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_rgba_resize(const ResizeArgs &args, hipStream_t stream)
{
    return launch_banded(k_rgba_resize, resize_plan, args, args.n_pictures, stream);
}

// ---------------------------------------------------------------------------------------
// k_tensor_resize: the area average of k_rgba_resize, normalised and stored as three planes of binary32, binary16 or bfloat16
// (tensor_resize_kernel.inl).  The launch shape is k_rgba_resize's: one wave per workgroup, no barrier, blockIdx.y = picture,
// blockIdx.z = segment of 64 output columns, blockIdx.x = band of RESIZE_ROWS output rows in XCD order.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_tensor_resize(TensorArgs a)
{
    __shared__ __attribute__((aligned(16))) ResizeLds lds;
    const uint32_t band = xcd_band(blockIdx.x, a.r.chunk);
    if (band >= a.r.bands) return;
    const int lane = threadIdx.x & 63;
    TensorLane t;
    tensor_resize_item(a, lds, band, blockIdx.z, blockIdx.y, [&](auto f) { f(lane, t); });
}

hipError_t launch_tensor_resize(const TensorArgs &args, hipStream_t stream)
{
    return launch_banded(k_tensor_resize, tensor_resize_plan, args, args.r.n_pictures, stream);
}

// ---------------------------------------------------------------------------------------
// k_rgba_resize_framed, k_tensor_resize_framed: a source window into a destination rectangle of the W' x H' output, the rest
// padded or kept (h263mi_framing; resize_kernel.inl, tensor_resize_kernel.inl).  Instantiations of their own: k_rgba_resize and
// k_tensor_resize above are not touched.  The launch shape is theirs over the W' x H' output: one wave per workgroup, no
// barrier, blockIdx.y = picture, blockIdx.z = segment of 64 output columns, blockIdx.x = band in XCD order.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_rgba_resize_framed(FramedResizeArgs a)
{
    __shared__ __attribute__((aligned(16))) ResizeLds lds;
    const uint32_t band = xcd_band(blockIdx.x, a.r.chunk);
    if (band >= a.r.bands) return;
    const int lane = threadIdx.x & 63;
    ResizeLane t;
    framed_resize_item(a, lds, band, blockIdx.z, blockIdx.y, [&](auto f) { f(lane, t); });
}

__global__ __launch_bounds__(64) void k_tensor_resize_framed(FramedTensorArgs a)
{
    __shared__ __attribute__((aligned(16))) ResizeLds lds;
    const uint32_t band = xcd_band(blockIdx.x, a.t.r.chunk);
    if (band >= a.t.r.bands) return;
    const int lane = threadIdx.x & 63;
    TensorLane t;
    framed_tensor_item(a, lds, band, blockIdx.z, blockIdx.y, [&](auto f) { f(lane, t); });
}

hipError_t launch_rgba_resize_framed(const FramedResizeArgs &args, hipStream_t stream)
{
    return launch_banded(k_rgba_resize_framed, framed_resize_plan, args, args.r.n_pictures, stream);
}

hipError_t launch_tensor_resize_framed(const FramedTensorArgs &args, hipStream_t stream)
{
    return launch_banded(k_tensor_resize_framed, framed_tensor_plan, args, args.t.r.n_pictures, stream);
}

// ---------------------------------------------------------------------------------------
// k_rgba_filter, k_tensor_filter: Pillow's bilinear / bicubic resampling of a source window into a destination rectangle of the
// W' x H' output, both passes in one kernel (h263mi_filter; filter_kernel.inl).  One instantiation each serves the framed and
// the unframed shapes.  The launch shape is that of the framed resizes over the W' x H' output: one wave per workgroup, no
// barrier, blockIdx.y = picture, blockIdx.z = segment of 64 output columns, blockIdx.x = band of FILTER_ROWS rows in XCD order.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_rgba_filter(FilterArgs a)
{
    __shared__ __attribute__((aligned(16))) FilterLds lds;
    const uint32_t band = xcd_band(blockIdx.x, a.chunk);
    if (band >= a.bands) return;
    const int lane = threadIdx.x & 63;
    FilterLane t;
    filter_rgba_item(a, lds, band, blockIdx.z, blockIdx.y, [&](auto f) { f(lane, t); });
}

__global__ __launch_bounds__(64) void k_tensor_filter(TensorFilterArgs a)
{
    __shared__ __attribute__((aligned(16))) FilterLds lds;
    const uint32_t band = xcd_band(blockIdx.x, a.fl.chunk);
    if (band >= a.fl.bands) return;
    const int lane = threadIdx.x & 63;
    TensorFilterLane t;
    filter_tensor_item(a, lds, band, blockIdx.z, blockIdx.y, [&](auto f) { f(lane, t); });
}

hipError_t launch_rgba_filter(const FilterArgs &args, hipStream_t stream)
{
    return launch_banded(k_rgba_filter, filter_rgba_plan, args, args.n_pictures, stream);
}

hipError_t launch_tensor_filter(const TensorFilterArgs &args, hipStream_t stream)
{
    return launch_banded(k_tensor_filter, filter_tensor_plan, args, args.fl.n_pictures, stream);
}

// ---------------------------------------------------------------------------------------
// k_plane_resize: area-average resampling of the full-size deblocked planes into I420 or NV12 (plane_resize_kernel.inl).  One
// wave per workgroup, no barrier; blockIdx.y = picture, blockIdx.z = segment of PLANE_OUT output columns (the luma segments,
// then the chroma segments: one launch for all planes), blockIdx.x = band of PLANE_ROWS output rows in XCD order, as
// k_rgba_resize.  A chroma wave whose band lies below its planes (they have half the rows) leaves at once.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_plane_resize(PlaneResizeArgs a)
{
    __shared__ __attribute__((aligned(16))) PlaneLds lds;
    const uint32_t band = xcd_band(blockIdx.x, a.chunk);
    if (band >= a.bands) return;
    const int lane = threadIdx.x & 63;
    PlaneLane t;
    plane_resize_item(a, lds, band, blockIdx.z, blockIdx.y, [&](auto f) { f(lane, t); });
}

hipError_t launch_plane_resize(const PlaneResizeArgs &args, hipStream_t stream)
{
    return launch_banded(k_plane_resize, plane_resize_plan, args, args.n_pictures, stream);
}

// ---------------------------------------------------------------------------------------
// k_plane_filter: Pillow's bilinear / bicubic resampling of the full-size deblocked planes into I420 or NV12, both passes in one
// kernel (plane_filter_kernel.inl).  The launch shape is k_plane_resize's: one wave per workgroup, no barrier; blockIdx.y =
// picture, blockIdx.z = segment of PLANE_OUT output columns (luma, then chroma), blockIdx.x = band of PFILTER_ROWS output rows in
// XCD order.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_plane_filter(PlaneFilterArgs a)
{
    __shared__ __attribute__((aligned(16))) PlaneFilterLds lds;
    const uint32_t band = xcd_band(blockIdx.x, a.chunk);
    if (band >= a.bands) return;
    const int lane = threadIdx.x & 63;
    PlaneFilterLane t;
    plane_filter_item(a, lds, band, blockIdx.z, blockIdx.y, [&](auto f) { f(lane, t); });
}

hipError_t launch_plane_filter(const PlaneFilterArgs &args, hipStream_t stream)
{
    return launch_banded(k_plane_filter, plane_filter_plan, args, args.n_pictures, stream);
}

// ---------------------------------------------------------------------------------------
// k_roi_tensor: a device table of regions of interest over full-size RGBA, each cut out and area-averaged into its own
// 3 x H' x W' tensor (h263mi_roi_tensor_on; roi_kernel.inl).  k_tensor_resize's launch shape with the region in the place of the
// picture: one wave per workgroup, no barrier, blockIdx.y = region, blockIdx.z = segment of 64 output columns, blockIdx.x = band
// of RESIZE_ROWS output rows in XCD order.  A wave validates its region and makes its spans itself.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_roi_tensor(RoiArgs a)
{
    __shared__ __attribute__((aligned(16))) ResizeLds lds;
    const uint32_t band = xcd_band(blockIdx.x, a.t.r.chunk);
    if (band >= a.t.r.bands) return;
    const int lane = threadIdx.x & 63;
    RoiLane t;
    roi_tensor_item(a, lds, band, blockIdx.z, blockIdx.y, [&](auto f) { f(lane, t); });
}

hipError_t launch_roi_tensor(const RoiArgs &args, hipStream_t stream)
{
    return launch_banded(k_roi_tensor, roi_plan, args, args.n_rois, stream);
}

}  // namespace h263mi
