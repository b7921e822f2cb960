"""ctypes binding of libh263mi.so (the C ABI of include/h263mi.h) for the tests and bench.py.

Python here is plumbing only: every compute call goes through the C ABI into the gfx950
kernels.  There is no fallback -- if the library or a GPU is missing, calls raise.

The class and function names mirror the reference API (ruffle-rs/h263-rs):
  H263State.decode_next_picture / get_last_picture / as_yuv   h263/src/decoder/state.rs
  deblock(data, width, strength), QUANT_TO_STRENGTH           deblock/src/deblock.rs:5-8,305
  yuv420_to_rgba(y, chroma_b, chroma_r, y_width)              yuv/src/bt601.rs:105
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("H263MI_LIB", os.path.join(_HERE, "libh263mi.so"))   # override: A/B runs of two builds

OK = 0
# h263/src/error.rs:6-58, in order (include/h263mi.h)
(ERR_INTERNAL_DECODER_ERROR, ERR_MIDDLE_OF_BITSTREAM, ERR_INVALID_MACROBLOCK_HEADER, ERR_INVALID_MACROBLOCK_CODED_BITS,
 ERR_INVALID_INTRA_DC, ERR_INVALID_SHORT_COEFFICIENT, ERR_INVALID_LONG_COEFFICIENT, ERR_INVALID_MVD, ERR_INVALID_PTYPE,
 ERR_INVALID_PLUS_PTYPE, ERR_INVALID_GOB_HEADER, ERR_INVALID_BITSTREAM, ERR_PICTURE_FORMAT_MISSING,
 ERR_PICTURE_FORMAT_INVALID, ERR_UNCODED_IFRAME_BLOCKS, ERR_UNHANDLED_IO_ERROR, ERR_UNIMPLEMENTED_DECODING) = range(-1, -18, -1)
ERR_INVALID_ARGUMENT = -100
ERR_NO_DEVICE = -101
ERR_HIP = -102
ERR_OUT_OF_MEMORY = -103
ERR_NO_PICTURE = -104

def events_from_dense(coeffs, intra_blocks=None):
    """dense (n, 64) LEVEL blocks -> (block_first_event, events) of h263mi_submit_picture_events.  intra_blocks: mask
    of blocks whose element 0 is not a TCOEF (the DC of an intra block travels in the record)."""
    c = np.ascontiguousarray(coeffs, np.int16).reshape(-1, 64)
    nz = c != 0
    if intra_blocks is not None:
        nz[np.asarray(intra_blocks, bool), 0] = False
    counts = nz.sum(axis=1)
    first = np.zeros(len(c) + 1, np.uint32)
    np.cumsum(counts, out=first[1:])
    blk, pos = np.nonzero(nz)
    ev = (c[blk, pos].astype(np.uint16).astype(np.uint32) << 16) | pos.astype(np.uint32)
    return first, ev


SORENSON_SPARK_BITSTREAM = 1
USE_SCALABILITY_MODE = 2
PICTURE_I, PICTURE_P, PICTURE_DISPOSABLE_P = 0, 1, 2
(PICTURE_RESERVED_SORENSON, PICTURE_PB, PICTURE_IMPROVED_PB, PICTURE_B, PICTURE_EI, PICTURE_EP,
 PICTURE_RESERVED) = range(3, 10)
SYNTH_I_DENSE, SYNTH_I_MIXED, SYNTH_P = 0, 1, 2

MB_RECORD_DTYPE = np.dtype([
    ("mb_type", "u1"), ("quant", "u1"), ("cbp", "u1"), ("kill", "u1"),
    ("mv", "<i2", (4, 2)), ("intradc", "u1", (6,)), ("reserved", "u1", (2,)),
    ("coeff_index", "<u4"),
])

EXPORTS = [
    "h263mi_strerror", "h263mi_abi_version",
    "h263mi_state_new", "h263mi_state_free", "h263mi_state_is_sorenson", "h263mi_state_reset",
    "h263mi_state_cleanup_buffers", "h263mi_submit_picture", "h263mi_decode_next_picture",
    "h263mi_parse_picture_header",
    "h263mi_get_last_picture", "h263mi_get_reference_picture", "h263mi_copy_yuv", "h263mi_render_rgba",
    "h263mi_quant_to_strength", "h263mi_deblock", "h263mi_bt601_yuv420_to_rgba", "h263mi_deblock_on",
    "h263mi_bt601_yuv420_to_rgba_on",
    "h263mi_batch_create", "h263mi_batch_destroy", "h263mi_batch_mbs_per_picture", "h263mi_batch_submit",
    "h263mi_batch_decode", "h263mi_batch_decode_events", "h263mi_batch_decode_next_pictures", "h263mi_batch_decode_next_pictures_ex",
    "h263mi_batch_sync_streams", "h263mi_batch_reset_stream", "h263mi_batch_set_active", "h263mi_batch_stream_has_picture",
    "h263mi_batch_render_rgba", "h263mi_batch_sync", "h263mi_batch_reset", "h263mi_batch_copy_yuv",
    "h263mi_batch_timing_begin", "h263mi_batch_timing_end", "h263mi_batch_timing_reserve", "h263mi_probe_bandwidth",
    "h263mi_probe_bandwidth_shape",
    "h263mi_batch_submit_host", "h263mi_submit_picture_events", "h263mi_batch_submit_host_events",
    "h263mi_device_count", "h263mi_device_malloc", "h263mi_device_free", "h263mi_device_memcpy_h2d",
    "h263mi_device_memcpy_d2h", "h263mi_device_synchronize",
    "h263mi_synth_picture_host", "h263mi_synth_batch_device", "h263mi_synth_batch_device_strided",
    "h263mi_default_parser_threads",
    "h263mi_render_rgba_pinned", "h263mi_host_alloc", "h263mi_host_free", "h263mi_host_register", "h263mi_host_unregister",
    "h263mi_debug_fail_nth_hip_call",
    "h263mi_mixed_create", "h263mi_mixed_destroy", "h263mi_mixed_decode_next_pictures", "h263mi_mixed_sync",
    "h263mi_mixed_stream_size", "h263mi_mixed_size_classes", "h263mi_mixed_set_memory_limit",
    "h263mi_mixed_frame_store_bytes", "h263mi_mixed_copy_yuv", "h263mi_mixed_reset_stream",
    # ABI 7: one post-filter strength per stream, explicit host share, NUMA placement report
    "h263mi_batch_decode_ps", "h263mi_batch_decode_events_ps", "h263mi_batch_render_rgba_ps",
    "h263mi_batch_decode_next_pictures_ps", "h263mi_mixed_decode_next_pictures_ps",
    "h263mi_set_ranks_per_node", "h263mi_batch_host_placement", "h263mi_debug_host_placement",
    # ABI 7, additive: scaled RGBA with a row pitch and per-stream placement
    "h263mi_rgba_layout_extent", "h263mi_batch_set_rgba_layout", "h263mi_render_rgba_layout",
    # ABI 7, additive: RGBA resized to any W' x H' by area averaging
    "h263mi_rgba_resize_extent", "h263mi_batch_set_rgba_resize", "h263mi_render_rgba_resize", "h263mi_mixed_set_rgba_resize",
    # ABI 7, additive: deblocked YUV 4:2:0 planes as I420 or NV12 with pitches and per-stream placement
    "h263mi_yuv_layout_extent", "h263mi_batch_set_yuv_layout", "h263mi_render_yuv",
    # ABI 7, additive: the same planes resized to any W' x H' by area averaging
    "h263mi_yuv_resize_extent", "h263mi_batch_set_yuv_resize", "h263mi_render_yuv_resize",
    # ABI 7, additive: Adler-32 digests of decoded pictures and output buffers, made on the device
    "h263mi_adler32_spans_on", "h263mi_batch_adler32_spans", "h263mi_digest_yuv", "h263mi_batch_digest_yuv",
    "h263mi_mixed_digest_yuv",
    # ABI 7, additive: the picture as a normalised planar float tensor (f32 / f16 / bf16) for inference
    "h263mi_tensor_extent", "h263mi_batch_set_tensor_output", "h263mi_render_tensor", "h263mi_mixed_set_tensor_output",
    # ABI 7, additive: aspect-preserving framing (letterbox, cover, window) of the resized RGBA and of the tensor
    "h263mi_framing_resolve", "h263mi_batch_set_rgba_resize_framed", "h263mi_batch_set_tensor_output_framed",
    "h263mi_render_rgba_resize_framed", "h263mi_render_tensor_framed", "h263mi_mixed_set_rgba_resize_framed",
    "h263mi_mixed_set_tensor_output_framed", "h263mi_mixed_stream_framing",
    # ABI 7, additive: bilinear and bicubic resampling (Pillow-exact) of the resized RGBA and of the tensor
    "h263mi_filter_taps", "h263mi_batch_set_rgba_resize_filtered", "h263mi_batch_set_tensor_output_filtered",
    "h263mi_render_rgba_resize_filtered", "h263mi_render_tensor_filtered", "h263mi_mixed_set_rgba_resize_filtered",
    "h263mi_mixed_set_tensor_output_filtered", "h263mi_batch_set_yuv_resize_filtered", "h263mi_render_yuv_resize_filtered",
    # ABI 7, additive: a device table of ROIs over full-size RGBA, cut out and resized into one tensor batch
    "h263mi_roi_tensor_on", "h263mi_batch_roi_tensor",
    # ABI 7, additive: change maps -- per-cell SAD of two plane sets, per-picture summaries, the list of changed pictures
    "h263mi_change_extent", "h263mi_change_map_on", "h263mi_batch_change_map", "h263mi_batch_change_last", "h263mi_change_last",
    # ABI 7, additive: plane histograms -- 256 counts per picture, statistics and percentiles, the list of scene cuts
    "h263mi_hist_extent", "h263mi_hist_on", "h263mi_batch_hist", "h263mi_batch_hist_last", "h263mi_hist_last",
    # ABI 7, additive: motion regions -- the changed cells of a change map's grids as a device table of ROI boxes
    "h263mi_regions_extent", "h263mi_regions_on", "h263mi_batch_regions",
    # ABI 7, additive: region tracks -- a table of ROI boxes matched from picture to picture, the tracks worth cropping as a table
    "h263mi_tracks_extent", "h263mi_tracks_on", "h263mi_batch_tracks",
    # ABI 7, additive: background model -- a running average per pixel and stream, foreground pixels counted per cell
    "h263mi_background_extent", "h263mi_background_on", "h263mi_batch_background", "h263mi_batch_background_last",
    "h263mi_background_last",
]
FILTER_AREA, FILTER_BILINEAR, FILTER_BICUBIC = 0, 1, 2
FRAME_STRETCH, FRAME_LETTERBOX, FRAME_COVER, FRAME_WINDOW = 0, 1, 2, 3
TENSOR_F32, TENSOR_F16, TENSOR_BF16 = 0, 1, 2
TENSOR_NUMPY_DTYPE = {TENSOR_F32: np.float32, TENSOR_F16: np.float16, TENSOR_BF16: np.uint16}     # (bfloat16: bit patterns)
YUV_I420, YUV_NV12 = 0, 1
STRENGTH_FROM_HEADER = 0xFF
CFG_OVERLAP_POST, CFG_PIPELINE_POST, CFG_TRUSTED_ARRAYS = 1, 2, 4


class H263Error(RuntimeError):
    def __init__(self, code, what=""):
        self.code = code
        msg = lib().h263mi_strerror(code).decode() if _lib is not None else str(code)
        super().__init__("%s: %s (%d)" % (what, msg, code))


class PictureDesc(C.Structure):
    _fields_ = [("width", C.c_uint16), ("height", C.c_uint16), ("picture_type", C.c_uint8), ("pquant", C.c_uint8),
                ("use_deblocker", C.c_uint8), ("reserved0", C.c_uint8), ("temporal_reference", C.c_uint16),
                ("reserved1", C.c_uint16)]


class BackendCfg(C.Structure):
    _fields_ = [("device_id", C.c_int32), ("flags", C.c_uint32), ("stream", C.c_void_p)]


class FrameView(C.Structure):
    _fields_ = [("width", C.c_uint16), ("height", C.c_uint16), ("chroma_width", C.c_uint16),
                ("chroma_height", C.c_uint16), ("temporal_reference", C.c_uint16), ("picture_type", C.c_uint8),
                ("pquant", C.c_uint8), ("use_deblocker", C.c_uint8), ("reserved", C.c_uint8 * 3),
                ("dev_y", C.c_void_p), ("dev_cb", C.c_void_p), ("dev_cr", C.c_void_p),
                ("dev_pitch_y", C.c_uint32), ("dev_pitch_c", C.c_uint32)]


class RgbaLayout(C.Structure):
    """h263mi_rgba_layout: output picture ceil(w / 2^scale_log2) x ceil(h / 2^scale_log2) box averages, rows row_pitch bytes
    apart (0 = tight), stream s's picture at byte offsets[s] (NULL = s * H' * pitch)."""
    _fields_ = [("scale_log2", C.c_uint8), ("reserved", C.c_uint8 * 7), ("row_pitch", C.c_uint64),
                ("offsets", C.POINTER(C.c_uint64))]


def make_rgba_layout(scale_log2=0, row_pitch=0, offsets=None):
    """-> (RgbaLayout, the offsets array it points into: keep it alive with the struct)"""
    lay = RgbaLayout()
    lay.scale_log2 = scale_log2
    lay.row_pitch = row_pitch
    keep = None
    if offsets is not None:
        keep = np.ascontiguousarray(offsets, dtype=np.uint64)
        lay.offsets = keep.ctypes.data_as(C.POINTER(C.c_uint64))
    return lay, keep


def rgba_layout_extent(n_streams, width, height, scale_log2=0, row_pitch=0, offsets=None, layout=None):
    """h263mi_rgba_layout_extent -> (W', H', bytes the output buffer must hold); H263Error when the layout is refused.
    layout: an RgbaLayout to pass as it is (else one is made of the other arguments)."""
    keep = None
    if layout is None:
        layout, keep = make_rgba_layout(scale_log2, row_pitch, offsets)
    ow, oh, nb = C.c_uint16(), C.c_uint16(), C.c_uint64()
    _check(lib().h263mi_rgba_layout_extent(n_streams, width, height, C.byref(layout), C.byref(ow), C.byref(oh), C.byref(nb)),
           "rgba_layout_extent")
    del keep
    return ow.value, oh.value, nb.value


class RgbaResize(C.Structure):
    """h263mi_rgba_resize: output picture out_width x out_height, the area average of the full-size RGBA, rows row_pitch bytes
    apart (0 = tight), stream s's picture at byte offsets[s] (NULL = s * H' * pitch)."""
    _fields_ = [("out_width", C.c_uint16), ("out_height", C.c_uint16), ("reserved", C.c_uint8 * 4), ("row_pitch", C.c_uint64),
                ("offsets", C.POINTER(C.c_uint64))]


def make_rgba_resize(out_width, out_height, row_pitch=0, offsets=None):
    """-> (RgbaResize, the offsets array it points into: keep it alive with the struct)"""
    r = RgbaResize()
    r.out_width = out_width
    r.out_height = out_height
    r.row_pitch = row_pitch
    keep = None
    if offsets is not None:
        keep = np.ascontiguousarray(offsets, dtype=np.uint64)
        r.offsets = keep.ctypes.data_as(C.POINTER(C.c_uint64))
    return r, keep


def rgba_resize_extent(n_streams, out_width, out_height, row_pitch=0, offsets=None, resize=None):
    """h263mi_rgba_resize_extent -> bytes the output buffer must hold; H263Error when the resize is refused.
    resize: an RgbaResize to pass as it is (else one is made of the other arguments)."""
    keep = None
    if resize is None:
        resize, keep = make_rgba_resize(out_width, out_height, row_pitch, offsets)
    nb = C.c_uint64()
    _check(lib().h263mi_rgba_resize_extent(n_streams, C.byref(resize), C.byref(nb)), "rgba_resize_extent")
    del keep
    return nb.value


class TensorOut(C.Structure):
    """h263mi_tensor_out: the picture as 3 planes of out_height x out_width elements of `dtype`, element = u * scale[colour] +
    bias[colour] (two binary32 roundings) of the area average u; strides in elements (0 = contiguous NCHW)."""
    _fields_ = [("out_width", C.c_uint16), ("out_height", C.c_uint16), ("dtype", C.c_uint8), ("bgr", C.c_uint8),
                ("reserved", C.c_uint8 * 2), ("scale", C.c_float * 3), ("bias", C.c_float * 3), ("stride_n", C.c_uint64),
                ("stride_c", C.c_uint64), ("stride_h", C.c_uint64)]


def make_tensor_out(out_width, out_height, dtype=TENSOR_F32, scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0), bgr=False, stride_n=0,
                    stride_c=0, stride_h=0):
    t = TensorOut()
    t.out_width, t.out_height, t.dtype, t.bgr = out_width, out_height, dtype, 1 if bgr else 0
    t.scale = (C.c_float * 3)(*[float(v) for v in scale])
    t.bias = (C.c_float * 3)(*[float(v) for v in bias])
    t.stride_n, t.stride_c, t.stride_h = stride_n, stride_c, stride_h
    return t


def tensor_extent(n_streams, tensor):
    """h263mi_tensor_extent -> bytes the tensor's buffer must hold; H263Error when the description is refused"""
    nb = C.c_uint64()
    _check(lib().h263mi_tensor_extent(n_streams, C.byref(tensor) if tensor is not None else None, C.byref(nb)), "tensor_extent")
    return nb.value


class Framing(C.Structure):
    """h263mi_framing: which rectangle of the picture fills which rectangle of the W' x H' output (FRAME_*), the colour around
    it (pad: R, G, B) or keep_outside; the rectangles are given under FRAME_WINDOW only."""
    _fields_ = [("mode", C.c_uint8), ("keep_outside", C.c_uint8), ("pad", C.c_uint8 * 3), ("reserved", C.c_uint8 * 3),
                ("src_x", C.c_uint16), ("src_y", C.c_uint16), ("src_w", C.c_uint16), ("src_h", C.c_uint16),
                ("dst_x", C.c_uint16), ("dst_y", C.c_uint16), ("dst_w", C.c_uint16), ("dst_h", C.c_uint16)]


class FramingRects(C.Structure):
    """h263mi_framing_rects: the resolved source and destination rectangles"""
    _fields_ = [(n, C.c_uint16) for n in ("src_x", "src_y", "src_w", "src_h", "dst_x", "dst_y", "dst_w", "dst_h")]

    def src(self):
        return (self.src_x, self.src_y, self.src_w, self.src_h)

    def dst(self):
        return (self.dst_x, self.dst_y, self.dst_w, self.dst_h)


def make_framing(mode=FRAME_STRETCH, pad=(0, 0, 0), keep_outside=False, src=None, dst=None):
    """-> Framing; src / dst: (x, y, w, h) of FRAME_WINDOW"""
    f = Framing()
    f.mode, f.keep_outside = mode, 1 if keep_outside else 0
    f.pad = (C.c_uint8 * 3)(*[int(v) for v in pad])
    if src is not None:
        f.src_x, f.src_y, f.src_w, f.src_h = src
    if dst is not None:
        f.dst_x, f.dst_y, f.dst_w, f.dst_h = dst
    return f


def _opt(struct):
    return C.byref(struct) if struct is not None else None


class Filter(C.Structure):
    """h263mi_filter: the resampling filter of a resized output (FILTER_AREA, FILTER_BILINEAR, FILTER_BICUBIC)"""
    _fields_ = [("kind", C.c_uint8), ("reserved", C.c_uint8 * 7)]


def make_filter(kind=FILTER_AREA):
    """-> Filter"""
    f = Filter()
    f.kind = kind
    return f


def filter_taps(kind, in_size, out_size):
    """h263mi_filter_taps -> (ksize, first[out_size], count[out_size], coeffs[out_size, ksize]): the source positions
    [first, first + count) that each output position reads and their weights in units of 2^-22 (no device); H263Error when the
    kind or a size is refused"""
    ks = C.c_uint32()
    _check(lib().h263mi_filter_taps(kind, in_size, out_size, C.byref(ks), None, None, None, 0), "filter_taps")
    first, count = np.zeros(out_size, np.uint32), np.zeros(out_size, np.uint32)
    coeffs = np.zeros((out_size, ks.value), np.int32)
    _check(lib().h263mi_filter_taps(kind, in_size, out_size, C.byref(ks), _p(first), _p(count), _p(coeffs), coeffs.size), "filter_taps")
    return ks.value, first, count, coeffs


def framing_resolve(width, height, out_width, out_height, framing=None):
    """h263mi_framing_resolve -> FramingRects of a width x height picture in an out_width x out_height output (no device);
    H263Error when the framing is refused.  A position of the output maps back to the source as
    x = src_x + (X - dst_x) * src_w / dst_w, y = src_y + (Y - dst_y) * src_h / dst_h."""
    rc = FramingRects()
    _check(lib().h263mi_framing_resolve(width, height, out_width, out_height, _opt(framing), C.byref(rc)), "framing_resolve")
    return rc


class YuvLayout(C.Structure):
    """h263mi_yuv_layout: the deblocked planes as I420 (Y, Cb, Cr) or NV12 (Y, interleaved CbCr), luma rows pitch_y bytes apart,
    chroma rows pitch_c (0 = tight), stream s's planes at byte offsets_y[s], offsets_cb[s], offsets_cr[s] (all NULL: back to back)."""
    _fields_ = [("format", C.c_uint8), ("reserved", C.c_uint8 * 7), ("pitch_y", C.c_uint64), ("pitch_c", C.c_uint64),
                ("offsets_y", C.POINTER(C.c_uint64)), ("offsets_cb", C.POINTER(C.c_uint64)), ("offsets_cr", C.POINTER(C.c_uint64))]


def make_yuv_layout(format=YUV_I420, pitch_y=0, pitch_c=0, offsets_y=None, offsets_cb=None, offsets_cr=None):
    """-> (YuvLayout, the offset arrays it points into: keep them alive with the struct)"""
    lay = YuvLayout()
    lay.format = format
    lay.pitch_y = pitch_y
    lay.pitch_c = pitch_c
    keep = []
    for name, offs in (("offsets_y", offsets_y), ("offsets_cb", offsets_cb), ("offsets_cr", offsets_cr)):
        if offs is not None:
            arr = np.ascontiguousarray(offs, dtype=np.uint64)
            setattr(lay, name, arr.ctypes.data_as(C.POINTER(C.c_uint64)))
            keep.append(arr)
    return lay, keep


def yuv_layout_extent(n_streams, width, height, format=YUV_I420, pitch_y=0, pitch_c=0, offsets_y=None, offsets_cb=None,
                      offsets_cr=None, layout=None, default=False):
    """h263mi_yuv_layout_extent -> bytes d_deblocked must hold; H263Error when the layout is refused.  Needs no device.
    layout: a YuvLayout to pass as it is (else one is made of the other arguments); default=True: the NULL layout."""
    keep = None
    if layout is None and not default:
        layout, keep = make_yuv_layout(format, pitch_y, pitch_c, offsets_y, offsets_cb, offsets_cr)
    nb = C.c_uint64()
    _check(lib().h263mi_yuv_layout_extent(n_streams, width, height, C.byref(layout) if layout is not None else None, C.byref(nb)),
           "yuv_layout_extent")
    del keep
    return nb.value


class YuvResize(C.Structure):
    """h263mi_yuv_resize: the deblocked planes resized to out_width x out_height (luma; chroma ceil(W'/2) x ceil(H'/2)), each
    plane the area average of its full-size plane, placed like a YuvLayout of an out_width x out_height picture."""
    _fields_ = [("out_width", C.c_uint16), ("out_height", C.c_uint16), ("format", C.c_uint8), ("reserved", C.c_uint8 * 3),
                ("pitch_y", C.c_uint64), ("pitch_c", C.c_uint64),
                ("offsets_y", C.POINTER(C.c_uint64)), ("offsets_cb", C.POINTER(C.c_uint64)), ("offsets_cr", C.POINTER(C.c_uint64))]


def make_yuv_resize(out_width, out_height, format=YUV_I420, pitch_y=0, pitch_c=0, offsets_y=None, offsets_cb=None,
                    offsets_cr=None):
    """-> (YuvResize, the offset arrays it points into: keep them alive with the struct)"""
    r = YuvResize()
    r.out_width = out_width
    r.out_height = out_height
    r.format = format
    r.pitch_y = pitch_y
    r.pitch_c = pitch_c
    keep = []
    for name, offs in (("offsets_y", offsets_y), ("offsets_cb", offsets_cb), ("offsets_cr", offsets_cr)):
        if offs is not None:
            arr = np.ascontiguousarray(offs, dtype=np.uint64)
            setattr(r, name, arr.ctypes.data_as(C.POINTER(C.c_uint64)))
            keep.append(arr)
    return r, keep


def yuv_resize_extent(n_streams, out_width, out_height, format=YUV_I420, pitch_y=0, pitch_c=0, offsets_y=None, offsets_cb=None,
                      offsets_cr=None, resize=None):
    """h263mi_yuv_resize_extent -> bytes d_deblocked must hold; H263Error when the resize is refused.  Needs no device.
    resize: a YuvResize to pass as it is (else one is made of the other arguments)."""
    keep = None
    if resize is None:
        resize, keep = make_yuv_resize(out_width, out_height, format, pitch_y, pitch_c, offsets_y, offsets_cb, offsets_cr)
    nb = C.c_uint64()
    _check(lib().h263mi_yuv_resize_extent(n_streams, C.byref(resize), C.byref(nb)), "yuv_resize_extent")
    del keep
    return nb.value


class DigestSpan(C.Structure):
    """h263mi_digest_span: `rows` rows of `row_bytes` bytes, `pitch` bytes apart, `offset` bytes behind the device pointer; the
    rows continue the byte string of output `digest` (non-decreasing over a table)."""
    _fields_ = [("offset", C.c_uint64), ("pitch", C.c_uint64), ("row_bytes", C.c_uint32), ("rows", C.c_uint32),
                ("digest", C.c_uint32), ("reserved", C.c_uint32)]


DIGEST_PIECE = 16384      # bytes one wave digests at most (csrc/digest_kernel.inl: DIGEST_PIECE); tests put sizes around it


def _span_array(spans):
    """DigestSpan instances or (offset, pitch, row_bytes, rows, digest) tuples -> (ctypes array or None, count)"""
    spans = list(spans)
    arr = (DigestSpan * max(len(spans), 1))()
    for i, sp in enumerate(spans):
        arr[i] = sp if isinstance(sp, DigestSpan) else DigestSpan(*sp)
    return (arr if spans else None), len(spans)


def _digest_count(spans, n_digests):
    if n_digests is not None:
        return n_digests
    return max([(sp.digest if isinstance(sp, DigestSpan) else sp[4]) for sp in spans], default=0) + 1


def adler32_spans(dev_ptr, buffer_bytes, spans, seed=1, n_digests=None, device_id=0, stream=None):
    """h263mi_adler32_spans_on: the Adler-32 (zlib.adler32(data, seed)) of the rows the spans name in the device buffer at dev_ptr,
    one per digest index (n_digests None: as many as the spans use) -> list of ints.  seed 1 is zlib's start value."""
    spans = list(spans)
    n_digests = _digest_count(spans, n_digests)
    arr, n = _span_array(spans)
    out = (C.c_uint32 * max(n_digests, 1))()
    cfg = BackendCfg(device_id, 0, stream)
    _check(lib().h263mi_adler32_spans_on(C.byref(cfg), dev_ptr, buffer_bytes, arr, n, seed, out, n_digests), "adler32_spans")
    return list(out)[:n_digests]


class Roi(C.Structure):
    """h263mi_roi: the rectangle (x, y, w, h) of full-size picture `picture`; reserved is 0"""
    _fields_ = [("picture", C.c_uint32), ("x", C.c_uint16), ("y", C.c_uint16), ("w", C.c_uint16), ("h", C.c_uint16),
                ("reserved", C.c_uint32)]


def roi_table(rois):
    """(picture, x, y, w, h[, reserved]) tuples -> the table as a (K, 4) uint32 array, 16 bytes a record: what is uploaded to
    the device (fields are cut to their widths, as a C caller's would be)"""
    out = np.zeros((len(rois), 4), np.uint32)
    for k, r in enumerate(rois):
        picture, x, y, w, h = r[:5]
        out[k] = (picture & 0xffffffff, (x & 0xffff) | (y & 0xffff) << 16, (w & 0xffff) | (h & 0xffff) << 16,
                  (r[5] if len(r) > 5 else 0) & 0xffffffff)
    return out


def roi_tensor(d_rgba, rgba_bytes, n_pictures, width, height, d_rois, n_rois, tensor, d_out, out_bytes, d_status=None, device_id=0,
               stream=None):
    """h263mi_roi_tensor_on: queues the launch that cuts the n_rois ROIs of the DEVICE table d_rois out of the full-size RGBA
    pictures at d_rgba into the tensor batch at d_out (extent: tensor_extent(n_rois, tensor)); does not wait.  d_status (device,
    n_rois words, or None): 0 per valid ROI, 1 per invalid one."""
    cfg = BackendCfg(device_id, 0, stream)
    _check(lib().h263mi_roi_tensor_on(C.byref(cfg), d_rgba, rgba_bytes, n_pictures, width, height, d_rois, n_rois, _opt(tensor), d_out,
                                      out_bytes, d_status), "roi_tensor")


class Change(C.Structure):
    """h263mi_change: cells of 1 << cell_log2 pixels (3..6); a cell is changed when sad * c*c > cell_threshold * pixels(cell); a
    picture is selected when changed_cells >= min_changed_cells; roll: prev takes cur's pixels"""
    _fields_ = [("cell_log2", C.c_uint8), ("roll", C.c_uint8), ("reserved", C.c_uint8 * 2), ("cell_threshold", C.c_uint32),
                ("min_changed_cells", C.c_uint32), ("reserved2", C.c_uint32)]


class PlaneSet(C.Structure):
    """h263mi_plane_set: `bytes` bytes of device memory at d_base; rows `pitch` apart, picture p's plane at p * picture_stride"""
    _fields_ = [("d_base", C.c_void_p), ("bytes", C.c_uint64), ("pitch", C.c_uint64), ("picture_stride", C.c_uint64)]


class ChangeSummary(C.Structure):
    _fields_ = [("sad", C.c_uint64), ("changed_cells", C.c_uint32), ("max_cell_sad", C.c_uint32)]


CHANGE_SUMMARY_DTYPE = np.dtype([("sad", np.uint64), ("changed_cells", np.uint32), ("max_cell_sad", np.uint32)])


def make_change(cell_log2=4, cell_threshold=0, min_changed_cells=1, roll=0):
    return Change(cell_log2, roll, (C.c_uint8 * 2)(0, 0), cell_threshold, min_changed_cells, 0)


def planes_default_set(d_deblocked, n_streams, w, h):
    """the luma planes of the tightly packed Y, Cb, Cr that a batch without a YUV layout writes to d_deblocked, as a PlaneSet"""
    picture = w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
    return PlaneSet(d_deblocked, n_streams * picture, w, picture)


def change_extent(n_pictures, width, height, change):
    """h263mi_change_extent -> (gw, gh, cells_bytes)"""
    gw, gh, nb = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
    _check(lib().h263mi_change_extent(n_pictures, width, height, _opt(change), C.byref(gw), C.byref(gh), C.byref(nb)), "change_extent")
    return gw.value, gh.value, nb.value


def change_map(cur, prev, n_pictures, width, height, change, d_cells, cells_bytes, d_summary, d_selected=None, d_count=None, device_id=0,
               stream=None):
    """h263mi_change_map_on: queues the launches that compare the PlaneSets cur and prev picture by picture -- cell SADs to d_cells
    (device, or None), a ChangeSummary per picture to d_summary, the ascending list of the pictures with changed_cells >=
    min_changed_cells to d_selected and its length to d_count (both device, or both None); does not wait."""
    cfg = BackendCfg(device_id, 0, stream)
    _check(lib().h263mi_change_map_on(C.byref(cfg), _opt(cur), _opt(prev), n_pictures, width, height, _opt(change), d_cells, cells_bytes,
                                      d_summary, d_selected, d_count), "change_map")


class Hist(C.Structure):
    """h263mi_hist: the percentiles p_lo and p_hi in permille; a picture is a cut when distance * 1000 > cut_permille * 2 * W*H; roll:
    prev takes the histograms"""
    _fields_ = [("roll", C.c_uint8), ("reserved", C.c_uint8 * 3), ("lo_permille", C.c_uint16), ("hi_permille", C.c_uint16),
                ("cut_permille", C.c_uint32), ("reserved2", C.c_uint32)]


class HistStats(C.Structure):
    _fields_ = [("sum", C.c_uint64), ("sum_sq", C.c_uint64), ("distance", C.c_uint64), ("min", C.c_uint8), ("max", C.c_uint8),
                ("p_lo", C.c_uint8), ("p_hi", C.c_uint8), ("mode", C.c_uint8), ("reserved", C.c_uint8 * 3)]


HIST_STATS_DTYPE = np.dtype([("sum", np.uint64), ("sum_sq", np.uint64), ("distance", np.uint64), ("min", np.uint8), ("max", np.uint8),
                             ("p_lo", np.uint8), ("p_hi", np.uint8), ("mode", np.uint8), ("reserved", np.uint8, (3,))])


def make_hist(lo_permille=10, hi_permille=990, cut_permille=500, roll=0):
    return Hist(roll, (C.c_uint8 * 3)(0, 0, 0), lo_permille, hi_permille, cut_permille, 0)


def hist_extent(n_pictures, width, height, hist):
    """h263mi_hist_extent -> hist_bytes"""
    nb = C.c_uint64(0)
    _check(lib().h263mi_hist_extent(n_pictures, width, height, _opt(hist), C.byref(nb)), "hist_extent")
    return nb.value


def hist(plane_set, n_pictures, width, height, hist, d_hist, hist_bytes, d_stats, d_prev_hist=None, prev_bytes=0, d_selected=None,
         d_count=None, device_id=0, stream=None):
    """h263mi_hist_on: queues the launches that count the PlaneSet's pictures -- 256 uint32 per picture to d_hist, a HistStats per
    picture to d_stats, the distance to d_prev_hist (device, or None), the ascending list of the cuts to d_selected and its length
    to d_count (both device, or both None); does not wait."""
    cfg = BackendCfg(device_id, 0, stream)
    _check(lib().h263mi_hist_on(C.byref(cfg), _opt(plane_set), n_pictures, width, height, _opt(hist), d_hist, hist_bytes, d_prev_hist,
                                prev_bytes, d_stats, d_selected, d_count), "hist")


REGIONS_MAX_CELLS = 32768


class Regions(C.Structure):
    """h263mi_regions: the grid's cell_log2 (3..6); connectivity 4 or 8; every box grows by margin_cells (0..8); a cell is changed by
    the rule of Change with cell_threshold; components of fewer than min_cells (>= 1) cells are dropped; at most max_per_picture
    (1..256) boxes a picture, the first in label order"""
    _fields_ = [("cell_log2", C.c_uint8), ("connectivity", C.c_uint8), ("margin_cells", C.c_uint8), ("reserved", C.c_uint8),
                ("cell_threshold", C.c_uint32), ("min_cells", C.c_uint32), ("max_per_picture", C.c_uint32)]


class RegionInfo(C.Structure):
    _fields_ = [("components", C.c_uint32), ("kept", C.c_uint32), ("first", C.c_uint32), ("written", C.c_uint32)]


class RegionStat(C.Structure):
    _fields_ = [("sad", C.c_uint64), ("cells", C.c_uint32), ("label", C.c_uint32)]


REGION_INFO_DTYPE = np.dtype([("components", np.uint32), ("kept", np.uint32), ("first", np.uint32), ("written", np.uint32)])
REGION_STAT_DTYPE = np.dtype([("sad", np.uint64), ("cells", np.uint32), ("label", np.uint32)])
ROI_DTYPE = np.dtype([("picture", np.uint32), ("x", np.uint16), ("y", np.uint16), ("w", np.uint16), ("h", np.uint16),
                      ("reserved", np.uint32)])


def make_regions(cell_log2=4, cell_threshold=0, connectivity=8, margin_cells=0, min_cells=1, max_per_picture=16):
    return Regions(cell_log2, connectivity, margin_cells, 0, cell_threshold, min_cells, max_per_picture)


def regions_extent(n_pictures, width, height, regions):
    """h263mi_regions_extent -> (gw, gh, cells_bytes, work_bytes)"""
    gw, gh, nb, wb = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
    _check(lib().h263mi_regions_extent(n_pictures, width, height, _opt(regions), C.byref(gw), C.byref(gh), C.byref(nb), C.byref(wb)),
           "regions_extent")
    return gw.value, gh.value, nb.value, wb.value


def regions(d_cells, cells_bytes, n_pictures, width, height, regions, d_work, work_bytes, d_rois, max_rois, d_info, d_count, d_stats=None,
            d_summary=None, device_id=0, stream=None):
    """h263mi_regions_on: queues the launches that turn the changed cells of the n_pictures grids at d_cells (as change_map writes
    them) into the table of Roi boxes at d_rois (max_rois entries, the unused ones invalid), a RegionStat per box at d_stats (or
    None), a RegionInfo per picture at d_info and the two count words at d_count; pictures whose ChangeSummary at d_summary (or
    None) has no changed cell are not read; d_work: work_bytes of staging (regions_extent); does not wait."""
    cfg = BackendCfg(device_id, 0, stream)
    _check(lib().h263mi_regions_on(C.byref(cfg), d_cells, cells_bytes, d_summary, n_pictures, width, height, _opt(regions), d_work,
                                   work_bytes, d_rois, max_rois, d_stats, d_info, d_count), "regions")


class Tracks(C.Structure):
    """h263mi_tracks: max_tracks (1..256) slots a picture; a pair is eligible from iou_permille (0..1000) on; a track dies behind
    max_missed (0..65534) consecutive misses; it is emitted from min_hits (>= 1) hits on: once (emit_period 0) or every
    emit_period-th hit"""
    _fields_ = [("max_tracks", C.c_uint16), ("iou_permille", C.c_uint16), ("max_missed", C.c_uint16), ("min_hits", C.c_uint16),
                ("emit_period", C.c_uint32), ("reserved", C.c_uint32)]


class Track(C.Structure):
    _fields_ = [("id", C.c_uint32), ("x", C.c_uint16), ("y", C.c_uint16), ("w", C.c_uint16), ("h", C.c_uint16), ("age", C.c_uint32),
                ("hits", C.c_uint32), ("missed", C.c_uint16), ("flags", C.c_uint16), ("det", C.c_uint32), ("reserved", C.c_uint32)]


class TrackHead(C.Structure):
    _fields_ = [("next_id", C.c_uint32), ("live", C.c_uint32), ("calls", C.c_uint32), ("reserved", C.c_uint32 * 5)]


class TrackInfo(C.Structure):
    _fields_ = [("detections", C.c_uint32), ("ignored", C.c_uint32), ("matched", C.c_uint32), ("born", C.c_uint32), ("died", C.c_uint32),
                ("dropped", C.c_uint32), ("first", C.c_uint32), ("written", C.c_uint32)]


class TrackRef(C.Structure):
    _fields_ = [("id", C.c_uint32), ("picture", C.c_uint32), ("hits", C.c_uint32), ("slot", C.c_uint16), ("flags", C.c_uint16)]


TRACK_DTYPE = np.dtype([("id", np.uint32), ("x", np.uint16), ("y", np.uint16), ("w", np.uint16), ("h", np.uint16), ("age", np.uint32),
                        ("hits", np.uint32), ("missed", np.uint16), ("flags", np.uint16), ("det", np.uint32), ("reserved", np.uint32)])
TRACK_HEAD_DTYPE = np.dtype([("next_id", np.uint32), ("live", np.uint32), ("calls", np.uint32), ("reserved", np.uint32, (5,))])
TRACK_INFO_DTYPE = np.dtype([(f, np.uint32) for f in ("detections", "ignored", "matched", "born", "died", "dropped", "first", "written")])
TRACK_REF_DTYPE = np.dtype([("id", np.uint32), ("picture", np.uint32), ("hits", np.uint32), ("slot", np.uint16), ("flags", np.uint16)])
TRACK_BORN, TRACK_MATCHED, TRACK_EMITTED = 1, 2, 4


def make_tracks(max_tracks=16, iou_permille=300, max_missed=2, min_hits=2, emit_period=0):
    return Tracks(max_tracks, iou_permille, max_missed, min_hits, emit_period, 0)


def tracks_extent(n_pictures, width, height, tracks):
    """h263mi_tracks_extent -> state_bytes"""
    nb = C.c_uint64(0)
    _check(lib().h263mi_tracks_extent(n_pictures, width, height, _opt(tracks), C.byref(nb)), "tracks_extent")
    return nb.value


def tracks(d_rois, n_rois, d_info_in, n_pictures, width, height, tracks, d_state, state_bytes, d_out_rois, max_out, d_info, d_count,
           d_out_refs=None, d_cut=None, d_cut_count=None, device_id=0, stream=None):
    """h263mi_tracks_on: queues the launches that update the n_pictures track states at d_state (tracks_extent; zeros: empty) from
    the table of Roi boxes at d_rois and its RegionInfo records at d_info_in (as regions writes them), and write the emitted tracks
    as Roi boxes to d_out_rois (max_out entries, the unused ones invalid), a TrackRef per box to d_out_refs (or None), a TrackInfo
    per picture to d_info and the two count words to d_count; the pictures listed at d_cut / d_cut_count (as hist writes d_selected
    / d_count; both or None) lose their tracks first; does not wait."""
    cfg = BackendCfg(device_id, 0, stream)
    _check(lib().h263mi_tracks_on(C.byref(cfg), d_rois, n_rois, d_info_in, n_pictures, width, height, _opt(tracks), d_state, state_bytes,
                                  d_cut, d_cut_count, d_out_rois, max_out, d_out_refs, d_info, d_count), "tracks")


class Background(C.Structure):
    """h263mi_background: cells as Change's; a pixel is foreground when it differs from its rounded background word by more than
    pixel_threshold; the word moves towards the pixel by the difference >> learn_shift (fg_learn_shift for a foreground pixel, 255:
    it keeps its word); nothing is foreground in the first `warmup` calls after an initialisation"""
    _fields_ = [("cell_log2", C.c_uint8), ("learn_shift", C.c_uint8), ("fg_learn_shift", C.c_uint8), ("pixel_threshold", C.c_uint8),
                ("warmup", C.c_uint16), ("reserved", C.c_uint16), ("cell_threshold", C.c_uint32), ("min_changed_cells", C.c_uint32)]


class BackgroundHead(C.Structure):
    _fields_ = [("age", C.c_uint32), ("mode", C.c_uint32), ("reserved", C.c_uint32 * 14)]


BACKGROUND_HEAD_DTYPE = np.dtype([("age", np.uint32), ("mode", np.uint32), ("reserved", np.uint32, (14,))])
BACKGROUND_VALID, BACKGROUND_INIT, BACKGROUND_WARM = 1, 2, 4
BACKGROUND_KEEP = 255


def make_background(cell_log2=4, learn_shift=4, fg_learn_shift=BACKGROUND_KEEP, pixel_threshold=24, warmup=0, cell_threshold=0,
                    min_changed_cells=1):
    return Background(cell_log2, learn_shift, fg_learn_shift, pixel_threshold, warmup, 0, cell_threshold, min_changed_cells)


def background_extent(n_pictures, width, height, background):
    """h263mi_background_extent -> (gw, gh, cells_bytes, state_bytes)"""
    gw, gh, nb, sb = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
    _check(lib().h263mi_background_extent(n_pictures, width, height, _opt(background), C.byref(gw), C.byref(gh), C.byref(nb), C.byref(sb)),
           "background_extent")
    return gw.value, gh.value, nb.value, sb.value


def background_on(cur, n_pictures, width, height, background, d_state, state_bytes, d_cells, cells_bytes, d_summary, d_selected=None,
                  d_count=None, mask=None, d_cut=None, d_cut_count=None, device_id=0, stream=None):
    """h263mi_background_on: queues the launches that judge every pixel of the PlaneSet cur against the n_pictures background
    states at d_state (background_extent; zeros: empty; a multiple of 32) and update them -- foreground counts per cell to d_cells
    (device, or None), a ChangeSummary per picture to d_summary, the list of the pictures with changed_cells >= min_changed_cells
    to d_selected / d_count (both or None), 255 / 0 per pixel to the PlaneSet mask (or None); the pictures listed at d_cut /
    d_cut_count (as hist writes d_selected / d_count; both or None) are initialised anew; does not wait."""
    cfg = BackendCfg(device_id, 0, stream)
    _check(lib().h263mi_background_on(C.byref(cfg), _opt(cur), n_pictures, width, height, _opt(background), d_state, state_bytes, d_cut,
                                      d_cut_count, _opt(mask), d_cells, cells_bytes, d_summary, d_selected, d_count), "background_on")


def _back_to_back(n_streams, picture_bytes):
    return [s * picture_bytes for s in range(n_streams)]


def spans_of_rgba(n_streams, out_w, out_h, row_pitch=0, offsets=None):
    """One digest per stream over its out_w x out_h RGBA picture in a buffer shaped by h263mi_rgba_layout / _resize: rows of
    4 * out_w bytes, row_pitch apart (0 = tight), stream s at offsets[s] (None: s * out_h * pitch)."""
    row = 4 * out_w
    pitch = row_pitch or row
    offs = _back_to_back(n_streams, out_h * pitch) if offsets is None else offsets
    return [DigestSpan(int(offs[s]), pitch, row, out_h, s, 0) for s in range(n_streams)]


def spans_of_yuv(n_streams, w, h, format=YUV_I420, pitch_y=0, pitch_c=0, offsets_y=None, offsets_cb=None, offsets_cr=None):
    """One digest per stream over its w x h planes in a buffer shaped by h263mi_yuv_layout / _resize: the Y rows, then the Cb rows,
    then the Cr rows (NV12: the Y rows, then the interleaved rows).  All offsets None: back to back, as h263mi_yuv_layout_extent."""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    row_c = cw if format == YUV_I420 else 2 * cw
    py, pc = pitch_y or w, pitch_c or row_c
    planes_c = 2 if format == YUV_I420 else 1
    if offsets_y is None:
        picture = h * py + planes_c * ch * pc
        offsets_y = _back_to_back(n_streams, picture)
        offsets_cb = [o + h * py for o in offsets_y]
        offsets_cr = [o + ch * pc for o in offsets_cb]
    out = []
    for s in range(n_streams):
        out.append(DigestSpan(int(offsets_y[s]), py, w, h, s, 0))
        out.append(DigestSpan(int(offsets_cb[s]), pc, row_c, ch, s, 0))
        if format == YUV_I420:
            out.append(DigestSpan(int(offsets_cr[s]), pc, cw, ch, s, 0))
    return out


def spans_of_planes_default(n_streams, w, h):
    """One digest per stream over the tightly packed Y, Cb, Cr that a batch without a YUV layout writes to d_deblocked"""
    return spans_of_yuv(n_streams, w, h, YUV_I420)


class KernelTimes(C.Structure):
    _fields_ = [("recon_ms", C.c_double), ("recon_launches", C.c_uint32), ("pad0", C.c_uint32),
                ("post_ms", C.c_double), ("post_launches", C.c_uint32), ("pad1", C.c_uint32),
                ("frame_ms", C.c_double), ("frame_launches", C.c_uint32), ("pad2", C.c_uint32)]


def build(force=False):
    """hipcc --offload-arch=gfx950 build of the shared library (h263-rs_amd/Makefile)."""
    if force:
        subprocess.check_call(["make", "-C", _HERE, "-s", "clean"])
    subprocess.check_call(["make", "-C", _HERE, "-s"])
    return LIB_PATH


_lib = None


class _MissingExport:
    argtypes = restype = None

    def __init__(self, name):
        self.name = name

    def __call__(self, *a):
        raise RuntimeError("%s: this build of libh263mi.so does not export %s" % (LIB_PATH, self.name))


def _has(name):
    return not isinstance(getattr(lib(), name, None), _MissingExport)


def lib():
    """Load the C-ABI library; fails loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libh263mi.so is missing: run `make -C h263-rs_amd` (hipcc, gfx950). "
                               "There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        # A library of an EARLIER round (tools/ab_inproc.py runs them beside HEAD) lacks the newer exports: a stand-in takes
        # the signature assignments below and raises when called.  (tests/test_abi.py holds HEAD's library to every export.)
        for name in EXPORTS:
            try:
                getattr(L, name)
            except AttributeError:
                setattr(L, name, _MissingExport(name))
        vp, sz, u8, u16, u32, i32 = C.c_void_p, C.c_size_t, C.c_uint8, C.c_uint16, C.c_uint32, C.c_int
        L.h263mi_strerror.restype = C.c_char_p
        L.h263mi_strerror.argtypes = [i32]
        L.h263mi_state_new.argtypes = [u32, C.POINTER(BackendCfg), C.POINTER(vp)]
        L.h263mi_state_free.argtypes = [vp]
        L.h263mi_state_free.restype = None
        L.h263mi_state_is_sorenson.argtypes = [vp]
        L.h263mi_state_reset.argtypes = [vp]
        L.h263mi_state_cleanup_buffers.argtypes = [vp]
        L.h263mi_submit_picture.argtypes = [vp, C.POINTER(PictureDesc), vp, sz, vp, sz]
        L.h263mi_submit_picture_events.argtypes = [vp, C.POINTER(PictureDesc), vp, sz, vp, sz, vp, sz]
        L.h263mi_decode_next_picture.argtypes = [vp, vp, sz, C.POINTER(sz)]
        L.h263mi_parse_picture_header.argtypes = [vp, vp, sz, C.POINTER(PictureDesc)]
        L.h263mi_get_last_picture.argtypes = [vp, C.POINTER(FrameView)]
        L.h263mi_get_reference_picture.argtypes = [vp, C.POINTER(FrameView)]
        L.h263mi_copy_yuv.argtypes = [vp, vp, vp, vp]
        L.h263mi_render_rgba.argtypes = [vp, u8, vp]
        L.h263mi_deblock.argtypes = [vp, sz, sz, u8, vp]
        L.h263mi_bt601_yuv420_to_rgba.argtypes = [vp, sz, vp, vp, sz, sz, vp]
        L.h263mi_batch_create.argtypes = [u32, u16, u16, C.POINTER(BackendCfg), C.POINTER(vp)]
        L.h263mi_batch_destroy.argtypes = [vp]
        L.h263mi_batch_destroy.restype = None
        L.h263mi_batch_mbs_per_picture.argtypes = [vp]
        L.h263mi_batch_mbs_per_picture.restype = u32
        L.h263mi_batch_submit.argtypes = [vp, u8, vp, vp, vp]
        L.h263mi_batch_decode.argtypes = [vp, u8, vp, vp, vp, C.c_uint64, u8, vp, vp]
        L.h263mi_batch_decode_events.argtypes = [vp, u8, vp, vp, vp, vp, C.c_uint64, C.c_uint64, u8, vp, vp]
        L.h263mi_render_rgba_pinned.argtypes = [vp, u8, vp]
        L.h263mi_host_alloc.argtypes = [sz, C.POINTER(vp)]
        L.h263mi_host_free.argtypes = [vp]
        L.h263mi_host_register.argtypes = [vp, sz]
        L.h263mi_host_unregister.argtypes = [vp]
        L.h263mi_debug_fail_nth_hip_call.argtypes = [i32]
        L.h263mi_mixed_create.argtypes = [u32, C.POINTER(BackendCfg), C.POINTER(vp)]
        L.h263mi_mixed_destroy.argtypes = [vp]
        L.h263mi_mixed_destroy.restype = None
        L.h263mi_mixed_decode_next_pictures.argtypes = [vp, u32, vp, vp, vp, u32, vp, u8, vp, vp, vp]
        L.h263mi_mixed_sync.argtypes = [vp, vp]
        L.h263mi_mixed_stream_size.argtypes = [vp, u32, C.POINTER(u16), C.POINTER(u16)]
        L.h263mi_mixed_size_classes.argtypes = [vp]
        L.h263mi_mixed_size_classes.restype = u32
        L.h263mi_mixed_set_memory_limit.argtypes = [vp, C.c_uint64]
        L.h263mi_mixed_frame_store_bytes.argtypes = [vp]
        L.h263mi_mixed_frame_store_bytes.restype = C.c_uint64
        L.h263mi_mixed_copy_yuv.argtypes = [vp, u32, vp, vp, vp]
        L.h263mi_mixed_reset_stream.argtypes = [vp, u32]
        L.h263mi_batch_decode_next_pictures.argtypes = [vp, u32, vp, vp, vp, u32]
        L.h263mi_batch_decode_next_pictures_ex.argtypes = [vp, u32, vp, vp, vp, u32, vp, u8, vp, vp]
        L.h263mi_batch_sync_streams.argtypes = [vp, vp]
        L.h263mi_batch_reset_stream.argtypes = [vp, u32]
        L.h263mi_batch_set_active.argtypes = [vp, vp]
        L.h263mi_batch_stream_has_picture.argtypes = [vp, u32]
        L.h263mi_batch_submit_host.argtypes = [vp, u8, vp, vp, vp, vp]
        L.h263mi_batch_submit_host_events.argtypes = [vp, u8, vp, vp, vp, vp, vp, vp]
        L.h263mi_batch_render_rgba.argtypes = [vp, u8, vp, vp]
        L.h263mi_batch_sync.argtypes = [vp]
        L.h263mi_batch_reset.argtypes = [vp]
        L.h263mi_batch_copy_yuv.argtypes = [vp, u32, vp, vp, vp]
        L.h263mi_batch_timing_begin.argtypes = [vp]
        L.h263mi_batch_timing_end.argtypes = [vp, C.POINTER(KernelTimes)]
        L.h263mi_batch_timing_reserve.argtypes = [vp, u32]
        L.h263mi_probe_bandwidth.argtypes = [C.POINTER(BackendCfg), i32, sz, i32, C.POINTER(C.c_double)]
        L.h263mi_probe_bandwidth_shape.argtypes = [C.POINTER(BackendCfg), i32, sz, i32, C.POINTER(C.c_double), C.POINTER(C.c_char_p)]
        L.h263mi_device_count.argtypes = [C.POINTER(i32)]
        L.h263mi_device_malloc.argtypes = [i32, sz, C.POINTER(vp)]
        L.h263mi_device_free.argtypes = [i32, vp]
        L.h263mi_device_memcpy_h2d.argtypes = [i32, vp, vp, sz]
        L.h263mi_device_memcpy_d2h.argtypes = [i32, vp, vp, sz]
        L.h263mi_device_synchronize.argtypes = [i32]
        L.h263mi_synth_picture_host.argtypes = [i32, u16, u16, u32, u32, vp, vp, sz, C.POINTER(sz)]
        L.h263mi_synth_batch_device.argtypes = [C.POINTER(BackendCfg), i32, u16, u16, u32, u32, u32, vp, vp, sz, vp,
                                                C.POINTER(sz)]
        L.h263mi_synth_batch_device_strided.argtypes = [C.POINTER(BackendCfg), i32, u16, u16, u32, u32, u32, u32, vp, vp, sz, vp,
                                                        C.POINTER(sz)]
        L.h263mi_batch_decode_ps.argtypes = [vp, u8, vp, vp, vp, C.c_uint64, u8, vp, vp, vp]
        L.h263mi_batch_decode_events_ps.argtypes = [vp, u8, vp, vp, vp, vp, C.c_uint64, C.c_uint64, u8, vp, vp, vp]
        L.h263mi_batch_render_rgba_ps.argtypes = [vp, u8, vp, vp, vp]
        L.h263mi_batch_decode_next_pictures_ps.argtypes = [vp, u32, vp, vp, vp, u32, vp, u8, vp, vp, vp]
        L.h263mi_mixed_decode_next_pictures_ps.argtypes = [vp, u32, vp, vp, vp, u32, vp, u8, vp, vp, vp, vp]
        L.h263mi_set_ranks_per_node.argtypes = [u32]
        L.h263mi_set_ranks_per_node.restype = None
        L.h263mi_batch_host_placement.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(u32), vp, u32]
        L.h263mi_debug_host_placement.argtypes = [vp, u32, i32, u32, C.c_char_p, C.POINTER(i32), vp, u32, C.POINTER(u32)]
        L.h263mi_rgba_layout_extent.argtypes = [u32, u16, u16, vp, C.POINTER(u16), C.POINTER(u16), C.POINTER(C.c_uint64)]
        L.h263mi_batch_set_rgba_layout.argtypes = [vp, vp]
        L.h263mi_render_rgba_layout.argtypes = [vp, u8, vp, vp]
        L.h263mi_rgba_resize_extent.argtypes = [u32, vp, C.POINTER(C.c_uint64)]
        L.h263mi_batch_set_rgba_resize.argtypes = [vp, vp]
        L.h263mi_render_rgba_resize.argtypes = [vp, u8, vp, vp]
        L.h263mi_mixed_set_rgba_resize.argtypes = [vp, vp]
        L.h263mi_yuv_layout_extent.argtypes = [u32, u16, u16, vp, C.POINTER(C.c_uint64)]
        L.h263mi_batch_set_yuv_layout.argtypes = [vp, vp]
        L.h263mi_render_yuv.argtypes = [vp, u8, vp, vp]
        L.h263mi_yuv_resize_extent.argtypes = [u32, vp, C.POINTER(C.c_uint64)]
        L.h263mi_batch_set_yuv_resize.argtypes = [vp, vp]
        L.h263mi_render_yuv_resize.argtypes = [vp, u8, vp, vp]
        L.h263mi_adler32_spans_on.argtypes = [C.POINTER(BackendCfg), vp, C.c_uint64, vp, u32, u32, vp, u32]
        L.h263mi_batch_adler32_spans.argtypes = [vp, vp, C.c_uint64, vp, u32, u32, vp, u32]
        L.h263mi_digest_yuv.argtypes = [vp, u32, C.POINTER(u32)]
        L.h263mi_batch_digest_yuv.argtypes = [vp, u32, vp, vp]
        L.h263mi_mixed_digest_yuv.argtypes = [vp, u32, vp, vp]
        L.h263mi_default_parser_threads.restype = u32
        L.h263mi_default_parser_threads.argtypes = [u32, C.POINTER(u32)]
        L.h263mi_tensor_extent.argtypes = [u32, vp, C.POINTER(C.c_uint64)]
        L.h263mi_batch_set_tensor_output.argtypes = [vp, vp]
        L.h263mi_render_tensor.argtypes = [vp, u8, vp, vp]
        L.h263mi_mixed_set_tensor_output.argtypes = [vp, vp]
        u16 = C.c_uint16
        L.h263mi_framing_resolve.argtypes = [u16, u16, u16, u16, vp, vp]
        L.h263mi_batch_set_rgba_resize_framed.argtypes = [vp, vp, vp]
        L.h263mi_batch_set_tensor_output_framed.argtypes = [vp, vp, vp]
        L.h263mi_render_rgba_resize_framed.argtypes = [vp, u8, vp, vp, vp]
        L.h263mi_render_tensor_framed.argtypes = [vp, u8, vp, vp, vp]
        L.h263mi_mixed_set_rgba_resize_framed.argtypes = [vp, vp, vp]
        L.h263mi_mixed_set_tensor_output_framed.argtypes = [vp, vp, vp]
        L.h263mi_mixed_stream_framing.argtypes = [vp, u32, vp]
        L.h263mi_filter_taps.argtypes = [u8, u32, u32, vp, vp, vp, vp, C.c_size_t]
        L.h263mi_batch_set_rgba_resize_filtered.argtypes = [vp, vp, vp, vp]
        L.h263mi_batch_set_tensor_output_filtered.argtypes = [vp, vp, vp, vp]
        L.h263mi_render_rgba_resize_filtered.argtypes = [vp, u8, vp, vp, vp, vp]
        L.h263mi_render_tensor_filtered.argtypes = [vp, u8, vp, vp, vp, vp]
        L.h263mi_mixed_set_rgba_resize_filtered.argtypes = [vp, vp, vp, vp]
        L.h263mi_mixed_set_tensor_output_filtered.argtypes = [vp, vp, vp, vp]
        L.h263mi_batch_set_yuv_resize_filtered.argtypes = [vp, vp, vp]
        L.h263mi_render_yuv_resize_filtered.argtypes = [vp, u8, vp, vp, vp]
        L.h263mi_roi_tensor_on.argtypes = [vp, vp, C.c_uint64, u32, u16, u16, vp, u32, vp, vp, C.c_uint64, vp]
        L.h263mi_batch_roi_tensor.argtypes = [vp, vp, C.c_uint64, vp, u32, vp, vp, C.c_uint64, vp]
        L.h263mi_change_extent.argtypes = [u32, u32, u32, vp, vp, vp, vp]
        L.h263mi_regions_extent.argtypes = [u32, u32, u32, vp, vp, vp, vp, vp]
        L.h263mi_regions_on.argtypes = [vp, vp, C.c_uint64, vp, u32, u32, u32, vp, vp, C.c_uint64, vp, u32, vp, vp, vp]
        L.h263mi_batch_regions.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, C.c_uint64, vp, u32, vp, vp, vp]
        L.h263mi_tracks_extent.argtypes = [u32, u32, u32, vp, vp]
        L.h263mi_tracks_on.argtypes = [vp, vp, u32, vp, u32, u32, u32, vp, vp, C.c_uint64, vp, vp, vp, u32, vp, vp, vp]
        L.h263mi_batch_tracks.argtypes = [vp, vp, u32, vp, vp, vp, C.c_uint64, vp, vp, vp, u32, vp, vp, vp]
        L.h263mi_change_map_on.argtypes = [vp, vp, vp, u32, u32, u32, vp, vp, C.c_uint64, vp, vp, vp]
        L.h263mi_batch_change_map.argtypes = [vp, vp, vp, vp, vp, C.c_uint64, vp, vp, vp]
        L.h263mi_batch_change_last.argtypes = [vp, vp, vp, vp, C.c_uint64, vp, vp, vp, vp]
        L.h263mi_change_last.argtypes = [vp, vp, vp, vp, C.c_uint64, vp, vp, vp]
        L.h263mi_background_extent.argtypes = [u32, u32, u32, vp, vp, vp, vp, vp]
        L.h263mi_background_on.argtypes = [vp, vp, u32, u32, u32, vp, vp, C.c_uint64, vp, vp, vp, vp, C.c_uint64, vp, vp, vp]
        L.h263mi_batch_background.argtypes = [vp, vp, vp, vp, C.c_uint64, vp, vp, vp, vp, C.c_uint64, vp, vp, vp]
        L.h263mi_batch_background_last.argtypes = [vp, vp, vp, C.c_uint64, vp, vp, vp, vp, C.c_uint64, vp, vp, vp, vp]
        L.h263mi_background_last.argtypes = [vp, vp, vp, C.c_uint64, vp, vp, vp, vp, C.c_uint64, vp, vp, vp]
        L.h263mi_hist_extent.argtypes = [u32, u32, u32, vp, vp]
        L.h263mi_hist_on.argtypes = [vp, vp, u32, u32, u32, vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp]
        L.h263mi_batch_hist.argtypes = [vp, vp, vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp]
        L.h263mi_batch_hist_last.argtypes = [vp, u32, vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp, vp]
        L.h263mi_hist_last.argtypes = [vp, u32, vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp]
        _lib = L
    return _lib


def _check(rc, what):
    if rc != OK:
        raise H263Error(rc, what)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def device_count():
    n = C.c_int(0)
    rc = lib().h263mi_device_count(C.byref(n))
    return n.value if rc == OK else 0


QUANT_TO_STRENGTH = None


def quant_to_strength():
    """deblock::QUANT_TO_STRENGTH (deblock.rs:5-8)."""
    return np.array((C.c_uint8 * 32).in_dll(lib(), "h263mi_quant_to_strength"), dtype=np.uint8)


def deblock(data, width, strength):
    """deblock::deblock(data, width, strength) -> Vec<u8> (deblock.rs:305), on the GPU."""
    data = np.ascontiguousarray(data, dtype=np.uint8).ravel()
    out = np.empty_like(data)
    _check(lib().h263mi_deblock(_p(data), data.size, width, strength, _p(out)), "deblock")
    return out


def yuv420_to_rgba(y, chroma_b, chroma_r, y_width):
    """yuv::bt601::yuv420_to_rgba(y, chroma_b, chroma_r, y_width) -> Vec<u8> (bt601.rs:105), on the GPU."""
    y = np.ascontiguousarray(y, dtype=np.uint8).ravel()
    cb = np.ascontiguousarray(chroma_b, dtype=np.uint8).ravel()
    cr = np.ascontiguousarray(chroma_r, dtype=np.uint8).ravel()
    if cb.size != cr.size:
        raise H263Error(ERR_INVALID_ARGUMENT, "yuv420_to_rgba")
    out = np.empty(y.size * 4, dtype=np.uint8)
    _check(lib().h263mi_bt601_yuv420_to_rgba(_p(y), y.size, _p(cb), _p(cr), cb.size, y_width, _p(out)),
           "yuv420_to_rgba")
    return out


class DecodedPicture:
    """Host-side copy of DecodedPicture (h263/src/decoder/picture.rs:8-58)."""

    def __init__(self, view, y, cb, cr):
        self.width, self.height = view.width, view.height
        self.chroma_width, self.chroma_height = view.chroma_width, view.chroma_height
        self.temporal_reference = view.temporal_reference
        self.picture_type = view.picture_type
        self.pquant = view.pquant
        self.use_deblocker = view.use_deblocker
        self._yuv = (y, cb, cr)

    def luma_samples_per_row(self):
        return self.width

    def chroma_samples_per_row(self):
        return self.chroma_width

    def as_luma(self):
        return self._yuv[0]

    def as_chroma_b(self):
        return self._yuv[1]

    def as_chroma_r(self):
        return self._yuv[2]

    def as_yuv(self):
        return self._yuv


class H263State:
    """H263State (h263/src/decoder/state.rs:16-490) over the C ABI."""

    def __init__(self, decoder_options=SORENSON_SPARK_BITSTREAM, device_id=0, stream=None, cfg_flags=0):
        self._h = C.c_void_p()
        self._cfg = BackendCfg(device_id, cfg_flags, stream)
        _check(lib().h263mi_state_new(decoder_options, C.byref(self._cfg), C.byref(self._h)), "H263State::new")

    def close(self):
        if self._h:
            lib().h263mi_state_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def is_sorenson(self):
        return bool(lib().h263mi_state_is_sorenson(self._h))

    def reset(self):
        _check(lib().h263mi_state_reset(self._h), "reset")

    def cleanup_buffers(self):
        _check(lib().h263mi_state_cleanup_buffers(self._h), "cleanup_buffers")

    def submit_picture(self, width, height, mbs, coeffs, picture_type=PICTURE_I, temporal_reference=0, pquant=1,
                       use_deblocker=0):
        """Record-level decode_next_picture (state.rs:421-483); raises H263Error on failure."""
        mbs = np.ascontiguousarray(mbs, dtype=MB_RECORD_DTYPE)
        coeffs = np.ascontiguousarray(coeffs, dtype=np.int16).reshape(-1, 64)
        d = PictureDesc(width, height, picture_type, pquant, use_deblocker, 0, temporal_reference, 0)
        _check(lib().h263mi_submit_picture(self._h, C.byref(d), _p(mbs) if mbs.size else None, mbs.size,
                                           _p(coeffs) if coeffs.size else None, coeffs.shape[0]), "submit_picture")

    def submit_picture_events(self, width, height, mbs, block_first_event, events, picture_type=PICTURE_I,
                              temporal_reference=0, pquant=1, use_deblocker=0):
        """submit_picture with sparse coefficient transport (h263mi_submit_picture_events)."""
        mbs = np.ascontiguousarray(mbs, dtype=MB_RECORD_DTYPE)
        first = np.ascontiguousarray(block_first_event, dtype=np.uint32)
        ev = np.ascontiguousarray(events, dtype=np.uint32)
        d = PictureDesc(width, height, picture_type, pquant, use_deblocker, 0, temporal_reference, 0)
        _check(lib().h263mi_submit_picture_events(self._h, C.byref(d), _p(mbs) if mbs.size else None, mbs.size, _p(first),
                                                  first.size - 1, _p(ev) if ev.size else None, ev.size),
               "submit_picture_events")

    def decode_next_picture(self, data):
        data = np.frombuffer(bytes(data), dtype=np.uint8)
        used = C.c_size_t(0)
        _check(lib().h263mi_decode_next_picture(self._h, _p(data), data.size, C.byref(used)), "decode_next_picture")
        return used.value

    def parse_picture(self, data):
        """H263State::parse_picture (state.rs:102-111): header fields of the picture that starts `data`."""
        data = np.frombuffer(bytes(data), dtype=np.uint8)
        d = PictureDesc()
        _check(lib().h263mi_parse_picture_header(self._h, _p(data), data.size, C.byref(d)), "parse_picture")
        return d

    def _view(self, fn, what):
        v = FrameView()
        rc = fn(self._h, C.byref(v))
        if rc == ERR_NO_PICTURE:
            return None
        _check(rc, what)
        return v

    def get_last_picture(self):
        """Option<&DecodedPicture> (state.rs:61-67): None before the first picture."""
        v = self._view(lib().h263mi_get_last_picture, "get_last_picture")
        if v is None:
            return None
        y = np.empty(v.width * v.height, np.uint8)
        cb = np.empty(v.chroma_width * v.chroma_height, np.uint8)
        cr = np.empty_like(cb)
        _check(lib().h263mi_copy_yuv(self._h, _p(y), _p(cb), _p(cr)), "as_yuv")
        return DecodedPicture(v, y, cb, cr)

    def has_reference_picture(self):
        return self._view(lib().h263mi_get_reference_picture, "get_reference_picture") is not None

    def digest_yuv(self, seed=1):
        """h263mi_digest_yuv: zlib.adler32(Y + Cb + Cr of the last picture, seed), made on the device"""
        d = C.c_uint32(0)
        _check(lib().h263mi_digest_yuv(self._h, seed, C.byref(d)), "digest_yuv")
        return d.value

    def change_last(self, prev, change, d_cells, cells_bytes, d_summary, d_selected=None, d_count=None):
        """h263mi_change_last: change_map with the last picture's luma, read in place, as cur (one picture); queues and returns"""
        _check(lib().h263mi_change_last(self._h, _opt(prev), _opt(change), d_cells, cells_bytes, d_summary, d_selected, d_count),
               "change_last")

    def background_last(self, background, d_state, state_bytes, d_cells, cells_bytes, d_summary, d_selected=None, d_count=None, mask=None,
                        d_cut=None, d_cut_count=None):
        """h263mi_background_last: background_on with the last picture's luma, read in place, as cur (one picture); queues and
        returns"""
        _check(lib().h263mi_background_last(self._h, _opt(background), d_state, state_bytes, d_cut, d_cut_count, _opt(mask), d_cells,
                                            cells_bytes, d_summary, d_selected, d_count), "background_last")

    def hist_last(self, plane, hist, d_hist, hist_bytes, d_stats, d_prev_hist=None, prev_bytes=0, d_selected=None, d_count=None):
        """h263mi_hist_last: hist() over plane `plane` (0 Y, 1 Cb, 2 Cr) of the last picture, read in place (one picture); queues
        and returns"""
        _check(lib().h263mi_hist_last(self._h, plane, _opt(hist), d_hist, hist_bytes, d_prev_hist, prev_bytes, d_stats, d_selected,
                                      d_count), "hist_last")

    def render_rgba(self, strength=0):
        v = self._view(lib().h263mi_get_last_picture, "get_last_picture")
        if v is None:
            raise H263Error(ERR_NO_PICTURE, "render_rgba")
        out = np.empty(v.width * v.height * 4, np.uint8)
        _check(lib().h263mi_render_rgba(self._h, strength, _p(out)), "render_rgba")
        return out

    def render_rgba_layout(self, strength, scale_log2=0, row_pitch=0):
        """h263mi_render_rgba_layout: H' * pitch bytes (rows of 4W' bytes; what lies between rows is zero here)"""
        v = self._view(lib().h263mi_get_last_picture, "get_last_picture")
        if v is None:
            raise H263Error(ERR_NO_PICTURE, "render_rgba_layout")
        ow, oh, nb = rgba_layout_extent(1, v.width, v.height, scale_log2, row_pitch)
        out = np.zeros(nb + (row_pitch - 4 * ow if row_pitch else 0), np.uint8)
        return self.render_rgba_layout_into(strength, out, scale_log2, row_pitch)

    def render_rgba_layout_into(self, strength, out, scale_log2=0, row_pitch=0):
        lay, _ = make_rgba_layout(scale_log2, row_pitch)
        _check(lib().h263mi_render_rgba_layout(self._h, strength, C.byref(lay), _p(out)), "render_rgba_layout")
        return out

    def render_rgba_resize(self, strength, out_width, out_height, row_pitch=0):
        """h263mi_render_rgba_resize: H' * pitch bytes (rows of 4W' bytes; what lies between rows is zero here)"""
        nb = rgba_resize_extent(1, out_width, out_height, row_pitch)
        out = np.zeros(nb + (row_pitch - 4 * out_width if row_pitch else 0), np.uint8)
        return self.render_rgba_resize_into(strength, out, out_width, out_height, row_pitch)

    def render_rgba_resize_into(self, strength, out, out_width, out_height, row_pitch=0):
        r, _ = make_rgba_resize(out_width, out_height, row_pitch)
        _check(lib().h263mi_render_rgba_resize(self._h, strength, C.byref(r), _p(out)), "render_rgba_resize")
        return out

    def render_rgba_resize_framed_into(self, strength, out, framing, out_width, out_height, row_pitch=0):
        """h263mi_render_rgba_resize_framed into `out`: with keep_outside its bytes outside the destination rectangle stay"""
        r, _ = make_rgba_resize(out_width, out_height, row_pitch)
        _check(lib().h263mi_render_rgba_resize_framed(self._h, strength, C.byref(r), _opt(framing), _p(out)), "render_rgba_resize_framed")
        return out

    def render_rgba_resize_framed(self, strength, framing, out_width, out_height, row_pitch=0):
        """h263mi_render_rgba_resize_framed: H' * pitch bytes (what no store reaches is zero here)"""
        out = np.zeros(rgba_resize_extent(1, out_width, out_height, row_pitch), np.uint8)
        return self.render_rgba_resize_framed_into(strength, out, framing, out_width, out_height, row_pitch)

    def render_tensor_framed_into(self, strength, tensor, framing, out):
        """h263mi_render_tensor_framed into `out` (an array whose first byte is the tensor's base)"""
        _check(lib().h263mi_render_tensor_framed(self._h, strength, C.byref(tensor), _opt(framing), _p(out)), "render_tensor_framed")
        return out

    def render_rgba_resize_filtered_into(self, strength, out, framing, filter, out_width, out_height, row_pitch=0):
        """h263mi_render_rgba_resize_filtered into `out` (framing, filter: None = none / the area average)"""
        r, _ = make_rgba_resize(out_width, out_height, row_pitch)
        _check(lib().h263mi_render_rgba_resize_filtered(self._h, strength, C.byref(r), _opt(framing), _opt(filter), _p(out)),
               "render_rgba_resize_filtered")
        return out

    def render_rgba_resize_filtered(self, strength, framing, filter, out_width, out_height, row_pitch=0):
        """h263mi_render_rgba_resize_filtered: H' * pitch bytes (what no store reaches is zero here)"""
        out = np.zeros(rgba_resize_extent(1, out_width, out_height, row_pitch), np.uint8)
        return self.render_rgba_resize_filtered_into(strength, out, framing, filter, out_width, out_height, row_pitch)

    def render_tensor_filtered_into(self, strength, tensor, framing, filter, out):
        """h263mi_render_tensor_filtered into `out` (an array whose first byte is the tensor's base)"""
        _check(lib().h263mi_render_tensor_filtered(self._h, strength, C.byref(tensor), _opt(framing), _opt(filter), _p(out)),
               "render_tensor_filtered")
        return out

    def render_tensor(self, strength, tensor):
        """h263mi_render_tensor -> a (3, H', W') array of float32 / float16, or of uint16 bit patterns for bfloat16, cut out of a
        buffer of the extent's size (what lies between rows and planes is zero there)"""
        nb = tensor_extent(1, tensor)
        dt = np.dtype(TENSOR_NUMPY_DTYPE[tensor.dtype])
        out = np.zeros(nb // dt.itemsize, dt)
        self.render_tensor_into(strength, tensor, out)
        W, H = tensor.out_width, tensor.out_height
        sh = tensor.stride_h or W
        sc = tensor.stride_c or H * sh
        return np.lib.stride_tricks.as_strided(out, (3, H, W), (sc * dt.itemsize, sh * dt.itemsize, dt.itemsize)).copy()

    def render_tensor_into(self, strength, tensor, out):
        """h263mi_render_tensor into `out` (an array whose first byte is the tensor's base); bytes outside the planes stay"""
        _check(lib().h263mi_render_tensor(self._h, strength, C.byref(tensor), _p(out)), "render_tensor")
        return out

    def render_yuv(self, strength=0, format=YUV_I420, pitch_y=0, pitch_c=0):
        """h263mi_render_yuv with default placement: the extent's bytes (what lies between rows is zero here)"""
        v = self._view(lib().h263mi_get_last_picture, "get_last_picture")
        if v is None:
            raise H263Error(ERR_NO_PICTURE, "render_yuv")
        out = np.zeros(yuv_layout_extent(1, v.width, v.height, format, pitch_y, pitch_c), np.uint8)
        return self.render_yuv_into(strength, out, format, pitch_y, pitch_c)

    def render_yuv_into(self, strength, out, format=YUV_I420, pitch_y=0, pitch_c=0, offsets_y=None, offsets_cb=None,
                        offsets_cr=None, layout=None):
        """h263mi_render_yuv into `out` (a uint8 array of at least the layout's extent); bytes outside the planes stay"""
        keep = None
        if layout is None:
            layout, keep = make_yuv_layout(format, pitch_y, pitch_c, offsets_y, offsets_cb, offsets_cr)
        _check(lib().h263mi_render_yuv(self._h, strength, C.byref(layout), _p(out)), "render_yuv")
        del keep
        return out

    def render_yuv_resize(self, strength, out_width, out_height, format=YUV_I420, pitch_y=0, pitch_c=0):
        """h263mi_render_yuv_resize with default placement: the extent's bytes (what lies between rows is zero here)"""
        out = np.zeros(yuv_resize_extent(1, out_width, out_height, format, pitch_y, pitch_c), np.uint8)
        return self.render_yuv_resize_into(strength, out, out_width, out_height, format, pitch_y, pitch_c)

    def render_yuv_resize_filtered(self, strength, filter, out_width, out_height, format=YUV_I420, pitch_y=0, pitch_c=0):
        """h263mi_render_yuv_resize_filtered with default placement: the extent's bytes (what lies between rows is zero here)"""
        out = np.zeros(yuv_resize_extent(1, out_width, out_height, format, pitch_y, pitch_c), np.uint8)
        return self.render_yuv_resize_filtered_into(strength, out, filter, out_width, out_height, format, pitch_y, pitch_c)

    def render_yuv_resize_filtered_into(self, strength, out, filter, out_width, out_height, format=YUV_I420, pitch_y=0, pitch_c=0,
                                        offsets_y=None, offsets_cb=None, offsets_cr=None, resize=None):
        """h263mi_render_yuv_resize_filtered into `out` (filter: a Filter, None = the area average); bytes outside the planes stay"""
        keep = None
        if resize is None:
            resize, keep = make_yuv_resize(out_width, out_height, format, pitch_y, pitch_c, offsets_y, offsets_cb, offsets_cr)
        _check(lib().h263mi_render_yuv_resize_filtered(self._h, strength, C.byref(resize), _opt(filter), _p(out)),
               "render_yuv_resize_filtered")
        del keep
        return out

    def render_yuv_resize_into(self, strength, out, out_width, out_height, format=YUV_I420, pitch_y=0, pitch_c=0, offsets_y=None,
                               offsets_cb=None, offsets_cr=None, resize=None):
        """h263mi_render_yuv_resize into `out` (a uint8 array of at least the resize's extent); bytes outside the planes stay"""
        keep = None
        if resize is None:
            resize, keep = make_yuv_resize(out_width, out_height, format, pitch_y, pitch_c, offsets_y, offsets_cb, offsets_cr)
        _check(lib().h263mi_render_yuv_resize(self._h, strength, C.byref(resize), _p(out)), "render_yuv_resize")
        del keep
        return out

    def render_rgba_pinned(self, strength, pinned):
        """h263mi_render_rgba_pinned: RGBA of the last picture straight into the caller's page-locked buffer (a PinnedBuffer
        or a registered numpy array); returns a view of the w*h*4 bytes"""
        v = self._view(lib().h263mi_get_last_picture, "get_last_picture")
        if v is None:
            raise H263Error(ERR_NO_PICTURE, "render_rgba_pinned")
        arr = pinned.array if isinstance(pinned, PinnedBuffer) else pinned
        n = v.width * v.height * 4
        assert arr.nbytes >= n
        _check(lib().h263mi_render_rgba_pinned(self._h, strength, _p(arr)), "render_rgba_pinned")
        return arr[:n]


class PinnedBuffer:
    """page-locked, device-visible host memory (h263mi_host_alloc) as a numpy uint8 array"""

    def __init__(self, nbytes):
        p = C.c_void_p()
        _check(lib().h263mi_host_alloc(nbytes, C.byref(p)), "host_alloc")
        self.ptr, self.nbytes = p.value, nbytes
        self.array = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(nbytes,))

    def free(self):
        if self.ptr:
            self.array = None
            lib().h263mi_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def host_register(arr):
    _check(lib().h263mi_host_register(_p(arr), arr.nbytes), "host_register")


def host_unregister(arr):
    _check(lib().h263mi_host_unregister(_p(arr)), "host_unregister")


def debug_fail_nth_hip_call(n):
    """TEST HOOK: the n-th HIP call of the host entry points from now on fails (0 = off); returns calls still to go"""
    return lib().h263mi_debug_fail_nth_hip_call(n)


def synchronize(device_id=0):
    _check(lib().h263mi_device_synchronize(device_id), "device_synchronize")


class DeviceBuffer:
    def __init__(self, nbytes, device_id=0):
        self.device_id, self.nbytes = device_id, nbytes
        self.ptr = C.c_void_p()
        _check(lib().h263mi_device_malloc(device_id, nbytes, C.byref(self.ptr)), "device_malloc")

    def upload(self, arr, offset=0):
        arr = np.ascontiguousarray(arr)
        assert offset + arr.nbytes <= self.nbytes
        _check(lib().h263mi_device_memcpy_h2d(self.device_id, C.c_void_p(self.ptr.value + offset), _p(arr),
                                              arr.nbytes), "h2d")

    def download(self, nbytes=None, offset=0, dtype=np.uint8):
        nbytes = self.nbytes - offset if nbytes is None else nbytes
        out = np.empty(nbytes, np.uint8)
        _check(lib().h263mi_device_memcpy_d2h(self.device_id, _p(out), C.c_void_p(self.ptr.value + offset), nbytes),
               "d2h")
        return out.view(dtype)

    def at(self, offset):
        return C.c_void_p(self.ptr.value + offset)

    def free(self):
        if self.ptr:
            lib().h263mi_device_free(self.device_id, self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Batch:
    """N independent streams advancing in lock step on one GPU (h263mi_batch_*)."""

    def __init__(self, n_streams, width, height, device_id=0, stream=None, overlap_post=False, pipeline_post=False,
                 trusted_arrays=False):
        """trusted_arrays: H263MI_CFG_TRUSTED_ARRAYS -- the caller vouches for the device arrays of submit / decode /
        decode_events; the default (ABI 7) bounds every one of them"""
        self.n, self.width, self.height, self.device_id = n_streams, width, height, device_id
        self._cfg = BackendCfg(device_id, (CFG_OVERLAP_POST if overlap_post else 0) | (CFG_PIPELINE_POST if pipeline_post else 0) |
                               (CFG_TRUSTED_ARRAYS if trusted_arrays else 0), stream)
        self._h = C.c_void_p()
        _check(lib().h263mi_batch_create(n_streams, width, height, C.byref(self._cfg), C.byref(self._h)),
               "batch_create")
        self.mbs_per_picture = lib().h263mi_batch_mbs_per_picture(self._h)

    def close(self):
        if self._h:
            lib().h263mi_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def submit(self, picture_type, d_mbs, d_coeffs, d_coeff_base=None):
        _check(lib().h263mi_batch_submit(self._h, picture_type, d_mbs, d_coeffs, d_coeff_base), "batch_submit")

    def _strengths(self, strengths):
        """None, or one post-filter strength per stream -> (keep-alive array, pointer) for the *_ps entry points"""
        if strengths is None:
            return None, None
        arr = np.ascontiguousarray(strengths, np.uint8)
        assert arr.size == self.n
        return arr, _p(arr)

    def decode(self, picture_type, d_mbs, d_coeffs, d_coeff_base=None, coeff_pool_blocks=0, strength=0, d_rgba=None,
               d_deblocked=None, strengths=None):
        """submit + render_rgba in one call (h263mi_batch_decode[_ps]).  strengths: one value per stream (ABI 7)"""
        keep, ps = self._strengths(strengths)
        if ps is None and not _has("h263mi_batch_decode_ps"):          # (a library of an earlier round: A/B runs)
            _check(lib().h263mi_batch_decode(self._h, picture_type, d_mbs, d_coeffs, d_coeff_base, coeff_pool_blocks, strength,
                                             d_rgba, d_deblocked), "batch_decode")
            return
        _check(lib().h263mi_batch_decode_ps(self._h, picture_type, d_mbs, d_coeffs, d_coeff_base, coeff_pool_blocks, strength, ps,
                                            d_rgba, d_deblocked), "batch_decode")

    def decode_events(self, picture_type, d_mbs, d_block_first_event, d_events, d_coeff_base=None, coeff_pool_blocks=0,
                      strength=0, d_rgba=None, d_deblocked=None, n_events=0, strengths=None):
        """h263mi_batch_decode_events[_ps]: decode with the coefficients as sparse events in device memory.  n_events: words
        in d_events, coeff_pool_blocks: blocks in the pool; a block whose bounds do not ascend or reach beyond them is not
        read and its picture is rejected.  0 = not told: the library bounds the arrays by the allocations they lie in (ABI 7)
        -- unless the batch was made with trusted_arrays, where 0 means the caller vouches and nothing is checked."""
        keep, ps = self._strengths(strengths)
        if ps is None and not _has("h263mi_batch_decode_events_ps"):
            _check(lib().h263mi_batch_decode_events(self._h, picture_type, d_mbs, d_block_first_event, d_events, d_coeff_base,
                                                    coeff_pool_blocks, n_events, strength, d_rgba, d_deblocked), "batch_decode_events")
            return
        _check(lib().h263mi_batch_decode_events_ps(self._h, picture_type, d_mbs, d_block_first_event, d_events, d_coeff_base,
                                                   coeff_pool_blocks, n_events, strength, ps, d_rgba, d_deblocked), "batch_decode_events")

    def decode_next_pictures(self, data_list, decoder_options=SORENSON_SPARK_BITSTREAM, n_threads=0, prepared=None):
        """one coded picture per stream (bytes-like objects) through the host parser threads and the GPU; returns the
        bytes consumed per stream.  `prepared` (from prepare_pictures) skips the per-call ctypes marshalling."""
        pd, ln, keep = prepared if prepared is not None else self.prepare_pictures(data_list)
        used = (C.c_size_t * self.n)()
        _check(lib().h263mi_batch_decode_next_pictures(self._h, decoder_options, pd, ln, used, n_threads),
               "batch_decode_next_pictures")
        return list(used)

    def prepare_pictures(self, data_list):
        """(None entries: the stream has no picture in the call -- decode_next_pictures_ex only)"""
        assert len(data_list) == self.n
        # an EMPTY picture (b"") is not "no picture": it goes to the parser and gets its end-of-stream error, so it
        # travels as a non-NULL pointer with length 0; only None becomes NULL
        empty = np.zeros(1, np.uint8)
        keep = [(np.frombuffer(bytes(d), dtype=np.uint8) if len(d) else empty) if d is not None else None for d in data_list]
        pd = (C.c_void_p * self.n)(*[k.ctypes.data if k is not None else None for k in keep])
        ln = (C.c_size_t * self.n)(*[(len(d) if d is not None else 0) for d in data_list])
        return pd, ln, keep

    def decode_next_pictures_ex(self, data_list, decoder_options=SORENSON_SPARK_BITSTREAM, n_threads=0, prepared=None,
                                strength=0, d_rgba=None, d_deblocked=None, strengths=None):
        """h263mi_batch_decode_next_pictures_ex / _ps: every stream its own H263State.  strength may be STRENGTH_FROM_HEADER
        (each picture with QUANT_TO_STRENGTH[its pquant] when its header sets USE_DEBLOCKER, else 0); strengths: one value
        per stream.  Returns (bytes consumed per stream, error code per stream: 0 = decoded or no data)."""
        pd, ln, keep = prepared if prepared is not None else self.prepare_pictures(data_list)
        used = (C.c_size_t * self.n)()
        rcs = (C.c_int * self.n)()
        keep_s, ps = self._strengths(strengths)
        _check(lib().h263mi_batch_decode_next_pictures_ps(self._h, decoder_options, pd, ln, used, n_threads, rcs, strength, ps,
                                                          d_rgba, d_deblocked), "batch_decode_next_pictures_ex")
        return list(used), list(rcs)

    def host_placement(self):
        """h263mi_batch_host_placement: (NUMA node of the device, node the pinned staging memory lies on, CPUs the host
        threads are confined to) -- -1 / -1 / [] where unknown or not made yet"""
        dn, sn, k = C.c_int(-1), C.c_int(-1), C.c_uint32(0)
        cpus = (C.c_uint16 * 1024)()
        _check(lib().h263mi_batch_host_placement(self._h, C.byref(dn), C.byref(sn), C.byref(k), cpus, 1024), "host_placement")
        return dn.value, sn.value, [int(cpus[i]) for i in range(min(k.value, 1024))]

    def sync_streams(self):
        """h263mi_batch_sync_streams: the device's verdict per stream (0 or an error code); never raises for those"""
        rcs = (C.c_int * self.n)()
        rc = lib().h263mi_batch_sync_streams(self._h, rcs)
        if rc != OK and not any(rcs):
            raise H263Error(rc, "batch_sync_streams")
        return list(rcs)

    def reset_stream(self, stream):
        _check(lib().h263mi_batch_reset_stream(self._h, stream), "batch_reset_stream")

    def set_active(self, active=None):
        arr = None if active is None else (C.c_uint8 * self.n)(*[1 if a else 0 for a in active])
        _check(lib().h263mi_batch_set_active(self._h, arr), "batch_set_active")

    def stream_has_picture(self, stream):
        return bool(lib().h263mi_batch_stream_has_picture(self._h, stream))

    def submit_host(self, picture_type, mbs_list, coeffs_list):
        """one picture per stream from host records: lists of MB_RECORD_DTYPE arrays and (n, 64) int16 arrays"""
        n = len(mbs_list)
        mbs = [np.ascontiguousarray(m, MB_RECORD_DTYPE) for m in mbs_list]
        cos = [np.ascontiguousarray(c, np.int16).reshape(-1, 64) for c in coeffs_list]
        pm = (C.c_void_p * n)(*[m.ctypes.data if m.size else None for m in mbs])
        pc = (C.c_void_p * n)(*[c.ctypes.data if c.size else None for c in cos])
        nm = (C.c_uint32 * n)(*[len(m) for m in mbs])
        nc = (C.c_uint32 * n)(*[len(c) for c in cos])
        _check(lib().h263mi_batch_submit_host(self._h, picture_type, pm, nm, pc, nc), "batch_submit_host")

    def submit_host_events(self, picture_type, mbs_list, first_list, events_list):
        """submit_host with sparse coefficient transport: per stream (block_first_event, events) arrays"""
        n = len(mbs_list)
        mbs = [np.ascontiguousarray(m, MB_RECORD_DTYPE) for m in mbs_list]
        fs = [np.ascontiguousarray(f, np.uint32) for f in first_list]
        evs = [np.ascontiguousarray(e, np.uint32) for e in events_list]
        pm = (C.c_void_p * n)(*[m.ctypes.data if m.size else None for m in mbs])
        pf = (C.c_void_p * n)(*[f.ctypes.data for f in fs])
        pe = (C.c_void_p * n)(*[e.ctypes.data if e.size else None for e in evs])
        nm = (C.c_uint32 * n)(*[len(m) for m in mbs])
        nb = (C.c_uint32 * n)(*[len(f) - 1 for f in fs])
        ne = (C.c_uint32 * n)(*[len(e) for e in evs])
        _check(lib().h263mi_batch_submit_host_events(self._h, picture_type, pm, nm, pf, nb, pe, ne), "batch_submit_host_events")

    def set_rgba_layout(self, scale_log2=0, row_pitch=0, offsets=None, default=False):
        """h263mi_batch_set_rgba_layout (default=True: back to today's layout)"""
        if default:
            _check(lib().h263mi_batch_set_rgba_layout(self._h, None), "batch_set_rgba_layout")
            return
        lay, keep = make_rgba_layout(scale_log2, row_pitch, offsets)
        _check(lib().h263mi_batch_set_rgba_layout(self._h, C.byref(lay)), "batch_set_rgba_layout")
        del keep

    def set_yuv_layout(self, format=YUV_I420, pitch_y=0, pitch_c=0, offsets_y=None, offsets_cb=None, offsets_cr=None,
                       default=False, layout=None):
        """h263mi_batch_set_yuv_layout: the shape of d_deblocked from now on (default=True: back to tightly packed I420)"""
        if default:
            _check(lib().h263mi_batch_set_yuv_layout(self._h, None), "batch_set_yuv_layout")
            return
        keep = None
        if layout is None:
            layout, keep = make_yuv_layout(format, pitch_y, pitch_c, offsets_y, offsets_cb, offsets_cr)
        _check(lib().h263mi_batch_set_yuv_layout(self._h, C.byref(layout)), "batch_set_yuv_layout")
        del keep

    def set_yuv_resize(self, out_width=0, out_height=0, format=YUV_I420, pitch_y=0, pitch_c=0, offsets_y=None, offsets_cb=None,
                       offsets_cr=None, default=False, resize=None):
        """h263mi_batch_set_yuv_resize: d_deblocked holds out_width x out_height planes from now on (default=True: back to
        tightly packed full-size I420)"""
        if default:
            _check(lib().h263mi_batch_set_yuv_resize(self._h, None), "batch_set_yuv_resize")
            return
        keep = None
        if resize is None:
            resize, keep = make_yuv_resize(out_width, out_height, format, pitch_y, pitch_c, offsets_y, offsets_cb, offsets_cr)
        _check(lib().h263mi_batch_set_yuv_resize(self._h, C.byref(resize)), "batch_set_yuv_resize")
        del keep

    def set_yuv_resize_filtered(self, resize, filter):
        """h263mi_batch_set_yuv_resize_filtered (resize: a YuvResize of make_yuv_resize, whose keep-alive the caller holds; None:
        back to tightly packed full-size I420.  filter: a Filter, None = the area average)"""
        _check(lib().h263mi_batch_set_yuv_resize_filtered(self._h, _opt(resize), _opt(filter)), "batch_set_yuv_resize_filtered")

    def set_rgba_resize(self, out_width=0, out_height=0, row_pitch=0, offsets=None, default=False):
        """h263mi_batch_set_rgba_resize (default=True: back to today's output)"""
        if default:
            _check(lib().h263mi_batch_set_rgba_resize(self._h, None), "batch_set_rgba_resize")
            return
        r, keep = make_rgba_resize(out_width, out_height, row_pitch, offsets)
        _check(lib().h263mi_batch_set_rgba_resize(self._h, C.byref(r)), "batch_set_rgba_resize")
        del keep

    def set_rgba_resize_framed(self, framing, out_width, out_height, row_pitch=0, offsets=None):
        """h263mi_batch_set_rgba_resize_framed (framing: a Framing, None = the plain resize)"""
        r, keep = make_rgba_resize(out_width, out_height, row_pitch, offsets)
        _check(lib().h263mi_batch_set_rgba_resize_framed(self._h, C.byref(r), _opt(framing)), "batch_set_rgba_resize_framed")
        del keep

    def set_tensor_output_framed(self, tensor, framing):
        """h263mi_batch_set_tensor_output_framed (tensor None: back to the default output; framing None: the plain tensor)"""
        _check(lib().h263mi_batch_set_tensor_output_framed(self._h, _opt(tensor), _opt(framing)), "batch_set_tensor_output_framed")

    def set_rgba_resize_filtered(self, framing, filter, out_width, out_height, row_pitch=0, offsets=None):
        """h263mi_batch_set_rgba_resize_filtered (framing None: none; filter: a Filter, None = the area average)"""
        r, keep = make_rgba_resize(out_width, out_height, row_pitch, offsets)
        _check(lib().h263mi_batch_set_rgba_resize_filtered(self._h, C.byref(r), _opt(framing), _opt(filter)),
               "batch_set_rgba_resize_filtered")
        del keep

    def set_tensor_output_filtered(self, tensor, framing, filter):
        """h263mi_batch_set_tensor_output_filtered (tensor None: back to the default output)"""
        _check(lib().h263mi_batch_set_tensor_output_filtered(self._h, _opt(tensor), _opt(framing), _opt(filter)),
               "batch_set_tensor_output_filtered")

    def set_tensor_output(self, tensor=None):
        """h263mi_batch_set_tensor_output: d_rgba of the later calls is the base of the tensor `tensor` (a TensorOut; None: back
        to today's output)"""
        _check(lib().h263mi_batch_set_tensor_output(self._h, C.byref(tensor) if tensor is not None else None), "batch_set_tensor_output")

    def render_rgba(self, strength, d_rgba, d_deblocked=None, strengths=None):
        keep, ps = self._strengths(strengths)
        _check(lib().h263mi_batch_render_rgba_ps(self._h, strength, ps, d_rgba, d_deblocked), "batch_render_rgba")

    def sync(self):
        _check(lib().h263mi_batch_sync(self._h), "batch_sync")

    def reset(self):
        _check(lib().h263mi_batch_reset(self._h), "batch_reset")

    def copy_yuv(self, stream):
        w, h = self.width, self.height
        cw, ch = (w + 1) // 2, (h + 1) // 2
        y, cb, cr = np.empty(w * h, np.uint8), np.empty(cw * ch, np.uint8), np.empty(cw * ch, np.uint8)
        _check(lib().h263mi_batch_copy_yuv(self._h, stream, _p(y), _p(cb), _p(cr)), "batch_copy_yuv")
        return y, cb, cr

    def digest_yuv(self, seed=1, stream_rc=True):
        """h263mi_batch_digest_yuv -> (digests, rcs): per stream zlib.adler32(Y + Cb + Cr of its last picture, seed) and 0, or 0 and
        ERR_NO_PICTURE.  stream_rc=None: no per-stream codes -- a stream without a picture raises ERR_NO_PICTURE; -> digests"""
        out = (C.c_uint32 * self.n)()
        rcs = (C.c_int * self.n)() if stream_rc is not None else None
        _check(lib().h263mi_batch_digest_yuv(self._h, seed, out, rcs), "batch_digest_yuv")
        return (list(out), list(rcs)) if rcs is not None else list(out)

    def adler32_spans(self, dev_ptr, buffer_bytes, spans, seed=1, n_digests=None):
        """h263mi_batch_adler32_spans: sync, then adler32_spans on the batch's device and stream -- for what the batch has written
        into d_rgba or d_deblocked (spans_of_rgba, spans_of_yuv, spans_of_planes_default)"""
        spans = list(spans)
        n_digests = _digest_count(spans, n_digests)
        arr, n = _span_array(spans)
        out = (C.c_uint32 * max(n_digests, 1))()
        _check(lib().h263mi_batch_adler32_spans(self._h, dev_ptr, buffer_bytes, arr, n, seed, out, n_digests), "batch_adler32_spans")
        return list(out)[:n_digests]

    def roi_tensor(self, d_rgba, rgba_bytes, d_rois, n_rois, tensor, d_out, out_bytes, d_status=None):
        """h263mi_batch_roi_tensor: sync, then roi_tensor on the batch's device and stream over the pictures it has written into
        d_rgba in the default shape"""
        _check(lib().h263mi_batch_roi_tensor(self._h, d_rgba, rgba_bytes, d_rois, n_rois, _opt(tensor), d_out, out_bytes, d_status),
               "batch_roi_tensor")

    def change_map(self, cur, prev, change, d_cells, cells_bytes, d_summary, d_selected=None, d_count=None):
        """h263mi_batch_change_map: sync, then change_map on the batch's device and stream with its picture size and stream count
        -- for two d_deblocked buffers a caller alternates between (planes_default_set)"""
        _check(lib().h263mi_batch_change_map(self._h, _opt(cur), _opt(prev), _opt(change), d_cells, cells_bytes, d_summary, d_selected,
                                             d_count), "batch_change_map")

    def change_last(self, prev, change, d_cells, cells_bytes, d_summary, d_selected=None, d_count=None, stream_rc=True):
        """h263mi_batch_change_last: change_map with the luma of every stream's last picture, read in place, as cur; queues and
        returns -> rcs (per stream 0 or ERR_NO_PICTURE).  stream_rc=None: a stream without a picture raises ERR_NO_PICTURE"""
        rcs = (C.c_int * self.n)() if stream_rc is not None else None
        _check(lib().h263mi_batch_change_last(self._h, _opt(prev), _opt(change), d_cells, cells_bytes, d_summary, d_selected, d_count,
                                              rcs), "batch_change_last")
        return list(rcs) if rcs is not None else None

    def background(self, cur, background, d_state, state_bytes, d_cells, cells_bytes, d_summary, d_selected=None, d_count=None, mask=None,
                   d_cut=None, d_cut_count=None):
        """h263mi_batch_background: sync, then background_on on the batch's device and stream with its picture size and stream
        count -- for a d_deblocked buffer (planes_default_set)"""
        _check(lib().h263mi_batch_background(self._h, _opt(cur), _opt(background), d_state, state_bytes, d_cut, d_cut_count, _opt(mask),
                                             d_cells, cells_bytes, d_summary, d_selected, d_count), "batch_background")

    def background_last(self, background, d_state, state_bytes, d_cells, cells_bytes, d_summary, d_selected=None, d_count=None, mask=None,
                        d_cut=None, d_cut_count=None, stream_rc=True):
        """h263mi_batch_background_last: background_on with the luma of every stream's last picture, read in place, as cur -- in
        change_last's place in front of regions; queues and returns -> rcs (per stream 0 or ERR_NO_PICTURE).  stream_rc=None: a
        stream without a picture raises ERR_NO_PICTURE"""
        rcs = (C.c_int * self.n)() if stream_rc is not None else None
        _check(lib().h263mi_batch_background_last(self._h, _opt(background), d_state, state_bytes, d_cut, d_cut_count, _opt(mask), d_cells,
                                                  cells_bytes, d_summary, d_selected, d_count, rcs), "batch_background_last")
        return list(rcs) if rcs is not None else None

    def hist(self, plane_set, hist, d_hist, hist_bytes, d_stats, d_prev_hist=None, prev_bytes=0, d_selected=None, d_count=None):
        """h263mi_batch_hist: sync, then hist() on the batch's device and stream with its picture size and stream count -- for a
        d_deblocked buffer (planes_default_set)"""
        _check(lib().h263mi_batch_hist(self._h, _opt(plane_set), _opt(hist), d_hist, hist_bytes, d_prev_hist, prev_bytes, d_stats,
                                       d_selected, d_count), "batch_hist")

    def hist_last(self, plane, hist, d_hist, hist_bytes, d_stats, d_prev_hist=None, prev_bytes=0, d_selected=None, d_count=None,
                  stream_rc=True):
        """h263mi_batch_hist_last: hist() over plane `plane` (0 Y, 1 Cb, 2 Cr) of every stream's last picture, read in place; queues
        and returns -> rcs (per stream 0 or ERR_NO_PICTURE).  stream_rc=None: a stream without a picture raises ERR_NO_PICTURE"""
        rcs = (C.c_int * self.n)() if stream_rc is not None else None
        _check(lib().h263mi_batch_hist_last(self._h, plane, _opt(hist), d_hist, hist_bytes, d_prev_hist, prev_bytes, d_stats,
                                            d_selected, d_count, rcs), "batch_hist_last")
        return list(rcs) if rcs is not None else None

    def regions(self, d_cells, cells_bytes, regions, d_work, work_bytes, d_rois, max_rois, d_info, d_count, d_stats=None, d_summary=None):
        """h263mi_batch_regions: sync, then regions() on the batch's device and stream with its picture size and stream count -- the
        step between change_last (same d_cells, d_summary) and roi_tensor (d_rois, n_rois = max_rois)"""
        _check(lib().h263mi_batch_regions(self._h, d_cells, cells_bytes, d_summary, _opt(regions), d_work, work_bytes, d_rois, max_rois,
                                          d_stats, d_info, d_count), "batch_regions")

    def tracks(self, d_rois, n_rois, d_info_in, tracks, d_state, state_bytes, d_out_rois, max_out, d_info, d_count, d_out_refs=None,
               d_cut=None, d_cut_count=None):
        """h263mi_batch_tracks: sync, then tracks() on the batch's device and stream with its picture size and stream count -- the
        step between regions (its d_rois, max_rois and d_info) and roi_tensor (d_out_rois, n_rois = max_out)"""
        _check(lib().h263mi_batch_tracks(self._h, d_rois, n_rois, d_info_in, _opt(tracks), d_state, state_bytes, d_cut, d_cut_count,
                                         d_out_rois, max_out, d_out_refs, d_info, d_count), "batch_tracks")

    def timing_begin(self):
        _check(lib().h263mi_batch_timing_begin(self._h), "timing_begin")

    def timing_reserve(self, n_launches):
        _check(lib().h263mi_batch_timing_reserve(self._h, n_launches), "timing_reserve")

    def timing_end(self):
        t = KernelTimes()
        _check(lib().h263mi_batch_timing_end(self._h, C.byref(t)), "timing_end")
        return t


PROBE_COPY, PROBE_READ, PROBE_WRITE = 0, 1, 2


class MixedBatch:
    """h263mi_mixed: n streams of different (and changing) picture sizes, one launch per size class and call"""

    def __init__(self, n_streams, device_id=0, stream=None, pipeline_post=False):
        cfg = BackendCfg(device_id, 2 if pipeline_post else 0, stream)
        h = C.c_void_p()
        _check(lib().h263mi_mixed_create(n_streams, C.byref(cfg), C.byref(h)), "mixed_create")
        self._h, self.n = h, n_streams

    def close(self):
        if self._h:
            lib().h263mi_mixed_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def decode_next_pictures(self, data_list, decoder_options=SORENSON_SPARK_BITSTREAM, n_threads=0, strength=0, rgba=None,
                             raise_on_error=True, strengths=None):
        """data_list: bytes or None per stream; rgba: DeviceBuffer or None per stream (or None: no rendering).
        Returns (bytes consumed, error codes, picture headers) per stream; with raise_on_error=False a call-level error
        does not raise and comes back as a fourth element (the per-stream results are valid either way)."""
        assert len(data_list) == self.n
        empty = np.zeros(1, np.uint8)
        keep = [(np.frombuffer(bytes(d), dtype=np.uint8) if len(d) else empty) if d is not None else None for d in data_list]
        pd = (C.c_void_p * self.n)(*[k.ctypes.data if k is not None else None for k in keep])
        ln = (C.c_size_t * self.n)(*[(len(d) if d is not None else 0) for d in data_list])
        used = (C.c_size_t * self.n)()
        rcs = (C.c_int * self.n)()
        descs = (PictureDesc * self.n)()
        ptrs = caps = None
        if rgba is not None:
            ptrs = (C.c_void_p * self.n)(*[(r.ptr.value if hasattr(r.ptr, "value") else r.ptr) if r is not None else None for r in rgba])
            caps = (C.c_size_t * self.n)(*[r.nbytes if r is not None else 0 for r in rgba])
        ps = None
        if strengths is not None:
            keep_s = np.ascontiguousarray(strengths, np.uint8)
            assert keep_s.size == self.n
            ps = _p(keep_s)
        rc = lib().h263mi_mixed_decode_next_pictures_ps(self._h, decoder_options, pd, ln, used, n_threads, rcs, strength, ps, ptrs, caps,
                                                        descs)
        if not raise_on_error:
            return list(used), list(rcs), list(descs), rc
        _check(rc, "mixed_decode_next_pictures")
        return list(used), list(rcs), list(descs)

    def sync(self):
        rcs = (C.c_int * self.n)()
        rc = lib().h263mi_mixed_sync(self._h, rcs)
        if rc != OK and not any(rcs):
            raise H263Error(rc, "mixed_sync")
        return list(rcs)

    def stream_size(self, stream):
        w, h = C.c_uint16(0), C.c_uint16(0)
        lib().h263mi_mixed_stream_size(self._h, stream, C.byref(w), C.byref(h))
        return w.value, h.value

    def size_classes(self):
        return lib().h263mi_mixed_size_classes(self._h)

    def set_rgba_resize(self, out_width=0, out_height=0, row_pitch=0, default=False):
        """h263mi_mixed_set_rgba_resize: every stream as out_width x out_height at its own buffer (default=True: full size)"""
        if default:
            _check(lib().h263mi_mixed_set_rgba_resize(self._h, None), "mixed_set_rgba_resize")
            return
        r, _ = make_rgba_resize(out_width, out_height, row_pitch)
        _check(lib().h263mi_mixed_set_rgba_resize(self._h, C.byref(r)), "mixed_set_rgba_resize")

    def set_rgba_resize_framed(self, framing, out_width, out_height, row_pitch=0):
        """h263mi_mixed_set_rgba_resize_framed: LETTERBOX / COVER resolved per size class (FRAME_WINDOW is refused)"""
        r, _ = make_rgba_resize(out_width, out_height, row_pitch)
        _check(lib().h263mi_mixed_set_rgba_resize_framed(self._h, C.byref(r), _opt(framing)), "mixed_set_rgba_resize_framed")

    def set_tensor_output_framed(self, tensor, framing):
        """h263mi_mixed_set_tensor_output_framed (tensor None: full-size RGBA again)"""
        _check(lib().h263mi_mixed_set_tensor_output_framed(self._h, _opt(tensor), _opt(framing)), "mixed_set_tensor_output_framed")

    def set_rgba_resize_filtered(self, framing, filter, out_width, out_height, row_pitch=0):
        """h263mi_mixed_set_rgba_resize_filtered: every size class with its own rectangle and its own tap tables"""
        r, _ = make_rgba_resize(out_width, out_height, row_pitch)
        _check(lib().h263mi_mixed_set_rgba_resize_filtered(self._h, C.byref(r), _opt(framing), _opt(filter)),
               "mixed_set_rgba_resize_filtered")

    def set_tensor_output_filtered(self, tensor, framing, filter):
        """h263mi_mixed_set_tensor_output_filtered (tensor None: full-size RGBA again)"""
        _check(lib().h263mi_mixed_set_tensor_output_filtered(self._h, _opt(tensor), _opt(framing), _opt(filter)),
               "mixed_set_tensor_output_filtered")

    def stream_framing(self, stream):
        """h263mi_mixed_stream_framing -> FramingRects of the stream's picture size under the shape in force"""
        rc = FramingRects()
        _check(lib().h263mi_mixed_stream_framing(self._h, stream, C.byref(rc)), "mixed_stream_framing")
        return rc

    def set_tensor_output(self, tensor=None):
        """h263mi_mixed_set_tensor_output: every stream as the 3 x H' x W' tensor `tensor` (stride_n 0) at its own buffer (None:
        full-size RGBA again)"""
        _check(lib().h263mi_mixed_set_tensor_output(self._h, C.byref(tensor) if tensor is not None else None), "mixed_set_tensor_output")

    def set_memory_limit(self, n_bytes):
        """what the frame stores of all size classes together may take (0 = no limit; default: half of the device's memory)"""
        _check(lib().h263mi_mixed_set_memory_limit(self._h, int(n_bytes)), "mixed_set_memory_limit")

    def frame_store_bytes(self):
        return int(lib().h263mi_mixed_frame_store_bytes(self._h))

    def copy_yuv(self, stream):
        w, h = self.stream_size(stream)
        if not w:
            raise H263Error(ERR_NO_PICTURE, "mixed_copy_yuv")
        cw, ch = (w + 1) // 2, (h + 1) // 2
        y, cb, cr = np.empty(w * h, np.uint8), np.empty(cw * ch, np.uint8), np.empty(cw * ch, np.uint8)
        _check(lib().h263mi_mixed_copy_yuv(self._h, stream, _p(y), _p(cb), _p(cr)), "mixed_copy_yuv")
        return y, cb, cr

    def digest_yuv(self, seed=1, stream_rc=True):
        """h263mi_mixed_digest_yuv -> (digests, rcs) as Batch.digest_yuv, one launch pair per size class"""
        out = (C.c_uint32 * self.n)()
        rcs = (C.c_int * self.n)() if stream_rc is not None else None
        _check(lib().h263mi_mixed_digest_yuv(self._h, seed, out, rcs), "mixed_digest_yuv")
        return (list(out), list(rcs)) if rcs is not None else list(out)

    def reset_stream(self, stream):
        _check(lib().h263mi_mixed_reset_stream(self._h, stream), "mixed_reset_stream")


MixedSet = MixedBatch


def probe_bandwidth(mode, nbytes=1 << 30, reps=10, device_id=0, stream=None, with_shape=False):
    """GB/s the device sustains for a streaming copy / read / write kernel: the fastest of the library's launch shapes
    (h263mi_probe_bandwidth); with_shape: (GB/s, description of the shape that won)."""
    cfg = BackendCfg(device_id, 0, stream)
    out = C.c_double(0.0)
    if with_shape:
        name = C.c_char_p()
        _check(lib().h263mi_probe_bandwidth_shape(C.byref(cfg), mode, nbytes, reps, C.byref(out), C.byref(name)), "probe_bandwidth")
        return out.value, (name.value or b"").decode()
    _check(lib().h263mi_probe_bandwidth(C.byref(cfg), mode, nbytes, reps, C.byref(out)), "probe_bandwidth")
    return out.value


def synth_picture_host(kind, width, height, stream_id, frame_idx):
    total = ((width + 15) // 16) * ((height + 15) // 16)
    mbs = np.zeros(total, MB_RECORD_DTYPE)
    coeffs = np.zeros((total * 6, 64), np.int16)
    n = C.c_size_t(0)
    _check(lib().h263mi_synth_picture_host(kind, width, height, stream_id, frame_idx, _p(mbs), _p(coeffs), total * 6,
                                           C.byref(n)), "synth_picture_host")
    return mbs, coeffs[:n.value].copy()


def debug_host_placement(pci_ids, device, ranks, sysfs_root=None):
    """h263mi_debug_host_placement (no GPU needed): (NUMA node, CPUs) a batch on `device` would be placed on"""
    arr = (C.c_char_p * len(pci_ids))(*[p.encode() for p in pci_ids])
    node, k = C.c_int(-1), C.c_uint32(0)
    cpus = (C.c_uint16 * 1024)()
    _check(lib().h263mi_debug_host_placement(arr, len(pci_ids), device, ranks, sysfs_root.encode() if sysfs_root else None,
                                             C.byref(node), cpus, 1024, C.byref(k)), "debug_host_placement")
    return node.value, [int(cpus[i]) for i in range(min(k.value, 1024))]


def set_ranks_per_node(ranks):
    """h263mi_set_ranks_per_node: how many processes share this node's CPUs with this one (0 = back to the environment)"""
    lib().h263mi_set_ranks_per_node(int(ranks))


def default_parser_threads(n_streams):
    """(threads, cpu_quota): the parser threads a batch call with n_threads = 0 uses for n_streams streams, and the CPU-time
    quota (in CPUs, 0 = none) that choice was made under (h263mi_default_parser_threads)."""
    q = C.c_uint32(0)
    t = lib().h263mi_default_parser_threads(n_streams, C.byref(q))
    return int(t), int(q.value)


def synth_batch_device(kind, width, height, n_streams, first_stream_id, frame_idx, d_mbs, d_coeffs, capacity_blocks,
                       d_coeff_base, device_id=0, stream=None, stream_stride=1):
    """picture p of the batch is stream first_stream_id + p * stream_stride"""
    cfg = BackendCfg(device_id, 0, stream)
    total = C.c_size_t(0)
    if stream_stride == 1 and not _has("h263mi_synth_batch_device_strided"):
        _check(lib().h263mi_synth_batch_device(C.byref(cfg), kind, width, height, n_streams, first_stream_id, frame_idx, d_mbs,
                                               d_coeffs, capacity_blocks, d_coeff_base, C.byref(total)), "synth_batch_device")
        return total.value
    _check(lib().h263mi_synth_batch_device_strided(C.byref(cfg), kind, width, height, n_streams, first_stream_id, stream_stride,
                                                   frame_idx, d_mbs, d_coeffs, capacity_blocks, d_coeff_base, C.byref(total)),
           "synth_batch_device")
    return total.value
