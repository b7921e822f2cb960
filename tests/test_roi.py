"""CPU side of the ROI crop-and-resize (h263mi_roi_tensor_on, h263mi_batch_roi_tensor): everything the host decides before any
device call -- the refusals in the order include/h263mi.h lists them, n_rois == 0, and the device check behind them.  The pointers
are made-up addresses: nothing here dereferences them, and a call that passes the argument checks names a device that no machine
has, so that it ends at the device check wherever the suite runs."""
import ctypes as C
import os

import pytest

import h263mi
import tensor_out_ref as tref

BAD, OK, NO_DEVICE = h263mi.ERR_INVALID_ARGUMENT, h263mi.OK, h263mi.ERR_NO_DEVICE
NO_GPU = not os.path.exists("/dev/kfd")
NOWHERE = h263mi.BackendCfg(1 << 20, 0, None)                       # a device id beyond any machine's
RGBA, ROIS, OUT, STATUS = 0x10000, 0x20000, 0x30000, 0x40000        # multiples of 16
W, H, N = 176, 144, 3


def call(tensor="default", rgba=RGBA, rgba_bytes=N * W * H * 4, n_pictures=N, width=W, height=H, rois=ROIS, n_rois=5, out=OUT,
         out_bytes=None, status=STATUS):
    t = h263mi.make_tensor_out(65, 5, h263mi.TENSOR_F16) if tensor == "default" else tensor
    if out_bytes is None:
        out_bytes = tref.extent(max(n_rois, 1), t.out_width, t.out_height, t.dtype, stride_n=t.stride_n, stride_c=t.stride_c,
                                stride_h=t.stride_h) if t is not None else 0
        out_bytes = out_bytes or 0
    return h263mi.lib().h263mi_roi_tensor_on(C.byref(NOWHERE), rgba, rgba_bytes, n_pictures, width, height, rois, n_rois,
                                             C.byref(t) if t is not None else None, out, out_bytes, status)


def test_the_structure_is_sixteen_bytes_and_the_table_packs_as_the_device_reads_it():
    assert C.sizeof(h263mi.Roi) == 16
    r = h263mi.Roi(7, 1, 2, 3, 4, 9)
    words = h263mi.roi_table([(7, 1, 2, 3, 4, 9)])
    assert bytes(r) == words.tobytes()
    assert h263mi.roi_table([(1, 65530, 0, 20, 10)]).tolist() == [[1, 65530, 20 | 10 << 16, 0]]


def test_refusals_in_order():
    # t NULL, or anything h263mi_tensor_extent refuses
    assert call(tensor=None) == BAD
    assert call(tensor=h263mi.make_tensor_out(0, 5)) == BAD
    assert call(tensor=h263mi.make_tensor_out(65, 5, 3)) == BAD
    assert call(tensor=h263mi.make_tensor_out(65, 5, stride_h=64)) == BAD
    assert call(tensor=h263mi.make_tensor_out(65, 5, scale=(1.0, float("inf"), 1.0))) == BAD
    small_n = h263mi.make_tensor_out(65, 5, stride_n=3 * 5 * 65 - 1)
    assert call(tensor=small_n, n_rois=2, out_bytes=1 << 20) == BAD               # the extent of n_rois tensors, not of one
    assert call(tensor=small_n, n_rois=1, out_bytes=1 << 20) == NO_DEVICE
    # n_pictures, width or height 0
    assert call(n_pictures=0, rgba_bytes=0) == BAD
    assert call(width=0) == BAD
    assert call(height=0) == BAD
    # width * height >= 2^30 (each side alone is fine)
    assert call(width=32768, height=32768, n_pictures=1, rgba_bytes=1 << 32) == BAD
    assert call(width=65535, height=16385, n_pictures=1, rgba_bytes=65535 * 16385 * 4) == BAD
    assert call(width=32769, height=32767, n_pictures=1, rgba_bytes=((1 << 30) - 1) * 4) == NO_DEVICE
    assert call(width=65535, height=1, n_pictures=1, rgba_bytes=65535 * 4) == NO_DEVICE     # not only decodable sizes
    # n_rois > 65535
    assert call(n_rois=65536, out_bytes=1 << 40) == BAD
    assert call(n_rois=65535, out_bytes=1 << 40) == NO_DEVICE
    # a NULL pointer while there are ROIs
    assert call(rgba=None) == BAD
    assert call(rois=None) == BAD
    assert call(out=None) == BAD
    assert call(status=None) == NO_DEVICE                                               # the status words are optional
    # alignment: the pictures to 16 bytes, the tensor to its element
    for off in (1, 2, 4, 8):
        assert call(rgba=RGBA + off) == BAD
    assert call(out=OUT + 1) == BAD
    assert call(out=OUT + 2) == NO_DEVICE                                               # (f16)
    assert call(tensor=h263mi.make_tensor_out(65, 5), out=OUT + 2) == BAD         # (f32)
    assert call(tensor=h263mi.make_tensor_out(65, 5), out=OUT + 4) == NO_DEVICE
    # the buffers hold what the call names
    assert call(rgba_bytes=N * W * H * 4 - 1) == BAD
    assert call(n_pictures=1 << 31, rgba_bytes=1 << 40) == BAD                    # (n_pictures * bytes does not wrap)
    full = tref.extent(5, 65, 5, tref.F16)
    assert call(out_bytes=full - 1) == BAD
    assert call(out_bytes=full) == NO_DEVICE


def test_an_earlier_refusal_wins_over_the_device_check_and_over_a_later_one():
    # everything wrong at once: still INVALID_ARGUMENT, never a device error
    assert call(tensor=None, rgba=None, n_pictures=0, n_rois=70000) == BAD


def test_no_rois_is_ok_without_a_launch_and_without_a_device():
    assert call(n_rois=0) == OK
    assert call(n_rois=0, rgba=None, rois=None, out=None, status=None, out_bytes=0) == OK
    # ... but the description is still looked at
    assert call(n_rois=0, tensor=None) == BAD
    assert call(n_rois=0, tensor=h263mi.make_tensor_out(65, 5, 7)) == BAD
    assert call(n_rois=0, width=0) == BAD
    assert call(n_rois=0, rgba=RGBA + 4) == BAD


def test_batch_call_refuses_no_batch():
    t = h263mi.make_tensor_out(65, 5)
    assert h263mi.lib().h263mi_batch_roi_tensor(None, RGBA, N * W * H * 4, ROIS, 5, C.byref(t), OUT, 1 << 20, None) == BAD


def test_a_valid_call_ends_at_the_device_check():
    assert call() == NO_DEVICE


@pytest.mark.skipif(not NO_GPU, reason="only meaningful where no GPU exists")
def test_a_valid_call_needs_a_device():
    t = h263mi.make_tensor_out(65, 5)
    assert h263mi.lib().h263mi_roi_tensor_on(None, RGBA, N * W * H * 4, N, W, H, ROIS, 5, C.byref(t), OUT, 1 << 20, STATUS) == NO_DEVICE
    with pytest.raises(h263mi.H263Error) as e:
        h263mi.roi_tensor(RGBA, N * W * H * 4, N, W, H, ROIS, 5, h263mi.make_tensor_out(65, 5), OUT, 1 << 20, STATUS)
    assert e.value.code == NO_DEVICE
