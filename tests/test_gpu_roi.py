"""GPU tests of the ROI crop-and-resize (h263mi_roi_tensor_on, h263mi_batch_roi_tensor: k_roi_tensor).  Every comparison is
exact, against roi_ref (framing_ref.rgba of the WINDOW, then tensor_out_ref.planes): output bits, status words and the sentinels
around the tensors.  The tables are the ones the kernel is run at lane by lane on the CPU (roi_cases.TABLES), where every hazard of
theirs is shown to occur.  The ROI table always reaches its device buffer through a device-side copy queued on the call's stream,
with no host wait between that copy and the call."""
import numpy as np
import pytest
import torch  # before the library is loaded: torch brings its own HIP runtime, which the C-ABI library must share (as in bench.py)

import framing_ref as fref
import h263mi
import roi_cases as rc
import roi_ref as ref
import tensor_out_ref as tref
from test_gpu_rgba_layout import _small_streams, _upload_records

pytestmark = pytest.mark.gpu
SENTINEL = 0xC3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if h263mi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")


@pytest.fixture(scope="module")
def stream():
    return torch.cuda.Stream(device=0)


_tables = {}


def table_data(name):
    """the table's pictures, uploaded with h263mi_device_memcpy_h2d, and the reference crops of its valid ROIs: made once"""
    if name not in _tables:
        (w, h), n, _, (ow, oh), rois = rc.TABLES[name]
        pics = rc.pictures(name)
        dev = h263mi.DeviceBuffer(n * w * h * 4)
        dev.upload(np.concatenate([p.ravel() for p in pics]))
        crops = [ref.crop(pics, r, ow, oh) if ref.valid(r, n, w, h) else None for r in rois]
        _tables[name] = (dev, crops)
    return _tables[name]


def _same(got, want, what):
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d elements differ, first at %s: %#x, want %#x" % (what, bad.size, bad[:8], got[bad[0]], want[bad[0]])


def _tensor_of(name, pl):
    _, _, _, (ow, oh), _ = rc.TABLES[name]
    return h263mi.make_tensor_out(ow, oh, pl["dtype"], pl["scale"], pl["bias"], bgr=pl["bgr"], stride_n=pl["arg_stride_n"],
                                  stride_c=pl["arg_stride_c"], stride_h=pl["arg_stride_h"])


def _sentinels(pl):
    et = tref.BITS_DTYPE[pl["dtype"]]
    return np.full(pl["elements"], np.array([SENTINEL] * 4, np.uint8).view(et)[0], et)


def _all_invalid(n):
    t = np.zeros((n, 4), np.uint32)
    t[:, 3] = 1                                               # reserved set: every record is refused
    return t


def _queue_table(stream, table, ballast=None):
    """the table into a device buffer that so far holds refused records only: staged in another device buffer, then copied on
    `stream` without waiting (behind `ballast`, a pair of large device tensors copied first) -> the device table (a torch tensor)"""
    words = np.ascontiguousarray(table).view(np.int32)
    staged = torch.from_numpy(words).cuda()
    d_rois = torch.from_numpy(_all_invalid(len(table)).view(np.int32)).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        if ballast is not None:
            ballast[1].copy_(ballast[0], non_blocking=True)
        d_rois.copy_(staged, non_blocking=True)
    return d_rois, staged


def _run_table(stream, name, which, ballast=None):
    (w, h), n, _, _, rois = rc.TABLES[name]
    dev, crops = table_data(name)
    pl = rc.placement(name, which)
    elt = tref.ELT[pl["dtype"]]
    t = _tensor_of(name, pl)
    assert h263mi.tensor_extent(len(rois), t) == pl["extent"] * elt
    canvas = _sentinels(pl)
    out = h263mi.DeviceBuffer(canvas.nbytes)
    out.upload(canvas)
    status = h263mi.DeviceBuffer(4 * len(rois) + 4)
    status.upload(np.full(len(rois) + 1, 0xC3C3C3C3, np.uint32))
    d_rois, keep = _queue_table(stream, h263mi.roi_table(rois), ballast)
    h263mi.roi_tensor(dev.ptr, dev.nbytes, n, w, h, d_rois.data_ptr(), len(rois), t, out.at(pl["base"] * elt), pl["extent"] * elt, status.ptr,
                      stream=stream.cuda_stream)
    stream.synchronize()
    want, want_status = ref.expected(canvas, crops, rois, n, w, h, pl["dtype"], pl["scale"], pl["bias"], pl["bgr"], pl["base"],
                                     pl["stride_n"], pl["stride_c"], pl["stride_h"])
    got_status = status.download(dtype=np.uint32)
    assert got_status[-1] == 0xC3C3C3C3
    _same(got_status[:-1], want_status, "%s %s: status" % (name, which))
    _same(out.download(dtype=canvas.dtype), want, "%s %s" % (name, which))
    out.free()
    status.free()
    del keep
    return want_status


# ---------------------------------------------------------------------------------------------
# 1. every table of the CPU checker, in every placement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(rc.PLACEMENTS))
@pytest.mark.parametrize("name", list(rc.TABLES))
def test_tables(stream, name, which):
    _run_table(stream, name, which)


def test_the_call_is_ordered_behind_a_copy_queued_on_its_stream(stream):
    """the table arrives behind 512 MiB of device-to-device copy on the same stream, the host waits for neither: a call that read
    the table early, or ran on another stream, would find the refused records that the buffer held before"""
    ballast = (torch.zeros(512 << 20, dtype=torch.uint8, device="cuda"), torch.empty(512 << 20, dtype=torch.uint8, device="cuda"))
    status = _run_table(stream, "qcif_65x5", "f16_odd_base_odd_stride", ballast)
    assert (status == 0).sum() >= 7                           # the valid ROIs of the table were seen as such


def test_no_status_words_and_no_rois(stream):
    name, which = "white_20x10", "bf16_contiguous"
    (w, h), n, _, _, rois = rc.TABLES[name]
    dev, crops = table_data(name)
    pl = rc.placement(name, which)
    t = _tensor_of(name, pl)
    canvas = _sentinels(pl)
    out = h263mi.DeviceBuffer(canvas.nbytes)
    out.upload(canvas)
    d_rois, keep = _queue_table(stream, h263mi.roi_table(rois))
    h263mi.roi_tensor(dev.ptr, dev.nbytes, n, w, h, d_rois.data_ptr(), 0, t, out.ptr, 0, None, stream=stream.cuda_stream)
    stream.synchronize()
    _same(out.download(dtype=canvas.dtype), canvas, "no ROIs")
    h263mi.roi_tensor(dev.ptr, dev.nbytes, n, w, h, d_rois.data_ptr(), len(rois), t, out.ptr, pl["extent"] * 2, None, stream=stream.cuda_stream)
    stream.synchronize()
    want, _ = ref.expected(canvas, crops, rois, n, w, h, pl["dtype"], pl["scale"], pl["bias"], pl["bgr"], 0, pl["stride_n"], pl["stride_c"],
                           pl["stride_h"])
    _same(out.download(dtype=canvas.dtype), want, "no status words")
    out.free()


def test_a_failure_of_the_runtime_is_reported_and_the_same_call_then_succeeds(stream):
    """the injected return code of h263mi_debug_fail_nth_hip_call: nothing faults on the device"""
    name, which = "odd_width_33x7", "f32_padded"
    (w, h), n, _, _, rois = rc.TABLES[name]
    dev, crops = table_data(name)
    pl = rc.placement(name, which)
    t = _tensor_of(name, pl)
    canvas = _sentinels(pl)
    out = h263mi.DeviceBuffer(canvas.nbytes)
    out.upload(canvas)
    d_rois, keep = _queue_table(stream, h263mi.roi_table(rois))
    call = lambda: h263mi.roi_tensor(dev.ptr, dev.nbytes, n, w, h, d_rois.data_ptr(), len(rois), t, out.at(pl["base"] * 4), pl["extent"] * 4,
                                     None, stream=stream.cuda_stream)
    h263mi.debug_fail_nth_hip_call(1)
    try:
        with pytest.raises(h263mi.H263Error) as e:
            call()
        assert h263mi.debug_fail_nth_hip_call(0) <= 0         # it fired: the call makes one HIP call, the launch
    finally:
        h263mi.debug_fail_nth_hip_call(0)
    assert e.value.code == h263mi.ERR_HIP
    stream.synchronize()
    _same(out.download(dtype=canvas.dtype), canvas, "after the failure")
    call()
    stream.synchronize()
    want, _ = ref.expected(canvas, crops, rois, n, w, h, pl["dtype"], pl["scale"], pl["bias"], pl["bgr"], pl["base"], pl["stride_n"],
                           pl["stride_c"], pl["stride_h"])
    _same(out.download(dtype=canvas.dtype), want, "the same call again")
    out.free()


# ---------------------------------------------------------------------------------------------
# 2. end to end: a batch decodes and renders in the default shape, the ROIs are cut out of what it wrote
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def qcif_batch_records():
    n, w, h = 3, 176, 144
    recs, _ = _upload_records(_small_streams(n, w, h, 8100), w, h)
    return n, w, h, recs


E2E_ROIS = [(2, 40, 30, 100, 90), (0, 0, 0, 176, 144), (1, 101, 77, 31, 19), (3, 0, 0, 8, 8), (1, 0, 0, 176, 144)]
E2E_OUT = (48, 40)


@pytest.mark.parametrize("mode", ["plain", "pipeline_post"])
def test_batch_roi_tensor_end_to_end(qcif_batch_records, mode):
    n, w, h, recs = qcif_batch_records
    ow, oh = E2E_OUT
    strength = 5
    scale, bias = tref.IMAGENET
    t = h263mi.make_tensor_out(ow, oh, tref.F16, scale, bias)
    nbytes = h263mi.tensor_extent(len(E2E_ROIS), t)
    b = h263mi.Batch(n, w, h, 0, None, pipeline_post=mode == "pipeline_post")
    rgba = h263mi.DeviceBuffer(n * w * h * 4)
    rgba.upload(np.full(rgba.nbytes, SENTINEL, np.uint8))
    out = h263mi.DeviceBuffer(nbytes)
    out.upload(np.full(nbytes, SENTINEL, np.uint8))
    status = h263mi.DeviceBuffer(4 * len(E2E_ROIS))
    d_rois = h263mi.DeviceBuffer(16 * len(E2E_ROIS))
    d_rois.upload(h263mi.roi_table(E2E_ROIS))
    b.decode(h263mi.PICTURE_I, recs[0].ptr, recs[1].ptr, recs[2].ptr, 0, strength, rgba.ptr, None)
    # (no sync here: a pipelined batch has only deferred its rendering -- the call delivers it)
    b.roi_tensor(rgba.ptr, rgba.nbytes, d_rois.ptr, len(E2E_ROIS), t, out.ptr, nbytes, status.ptr)
    b.sync()
    full = rgba.download().reshape(n, h, w, 4)
    assert not (full == SENTINEL).all(axis=(1, 2, 3)).any()  # every picture was rendered
    pics = [full[s] for s in range(n)]
    crops = [ref.crop(pics, r, ow, oh) if ref.valid(r, n, w, h) else None for r in E2E_ROIS]
    canvas = np.full(nbytes // 2, np.array([SENTINEL] * 2, np.uint8).view(np.uint16)[0], np.uint16)
    want, want_status = ref.expected(canvas, crops, E2E_ROIS, n, w, h, tref.F16, scale, bias, False, 0, 3 * oh * ow, oh * ow, ow)
    _same(status.download(dtype=np.uint32), want_status, "status")
    assert list(want_status) == [0, 0, 0, 1, 0]
    got = out.download(dtype=np.uint16)
    _same(got, want, mode)
    b.close()
    # ROI 0 against the bytes of the batch's own framed tensor output with the same WINDOW
    k = 0
    p, x, y, rw, rh = E2E_ROIS[k]
    b2 = h263mi.Batch(n, w, h, 0, None)
    b2.set_tensor_output_framed(t, h263mi.make_framing(fref.WINDOW, src=(x, y, rw, rh), dst=(0, 0, ow, oh)))
    framed = h263mi.DeviceBuffer(h263mi.tensor_extent(n, t))
    b2.decode(h263mi.PICTURE_I, recs[0].ptr, recs[1].ptr, recs[2].ptr, 0, strength, framed.ptr, None)
    b2.sync()
    one = 3 * oh * ow
    _same(got[k * one:(k + 1) * one], framed.download(dtype=np.uint16)[p * one:(p + 1) * one], "against the framed output")
    b2.close()
