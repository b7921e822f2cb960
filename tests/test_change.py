"""CPU side of the change maps (h263mi_change_extent, h263mi_change_map_on, h263mi_batch_change_map, h263mi_batch_change_last,
h263mi_change_last): everything the host decides before any device call -- the extent, every refusal include/h263mi.h lists,
n_pictures == 0, and the device check behind them.  The pointers are made-up addresses: nothing here dereferences them, and a call
that passes the argument checks names a device that no machine has, so that it ends at the device check wherever the suite runs."""
import ctypes as C
import os

import pytest

import h263mi

BAD, OK, NO_DEVICE = h263mi.ERR_INVALID_ARGUMENT, h263mi.OK, h263mi.ERR_NO_DEVICE
NO_GPU = not os.path.exists("/dev/kfd")
NOWHERE = h263mi.BackendCfg(1 << 20, 0, None)                       # a device id beyond any machine's
CUR, PREV, CELLS, SUMMARY, LIST, COUNT = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000
W, H, N = 100, 60, 3
DEFAULT = object()


def plane_set(base=CUR, w=W, h=H, n=N, pitch=None, stride=None, nbytes=None):
    pitch = w if pitch is None else pitch
    stride = h * pitch if stride is None else stride
    nbytes = (n - 1) * stride + (h - 1) * pitch + w if nbytes is None else nbytes
    return h263mi.PlaneSet(base, nbytes, pitch, stride)


def call(cur=DEFAULT, prev=DEFAULT, n=N, w=W, h=H, change=DEFAULT, cells=CELLS, cells_bytes=None, summary=SUMMARY, selected=LIST,
         count=COUNT):
    cur = plane_set(CUR, w, h, max(n, 1)) if cur is DEFAULT else cur
    prev = plane_set(PREV, w, h, max(n, 1)) if prev is DEFAULT else prev
    change = h263mi.make_change() if change is DEFAULT else change
    if cells_bytes is None:
        cl = change.cell_log2 if change is not None and 3 <= change.cell_log2 <= 6 else 4
        cells_bytes = n * -(-w // (1 << cl)) * -(-h // (1 << cl)) * 4
    return h263mi.lib().h263mi_change_map_on(C.byref(NOWHERE), h263mi._opt(cur), h263mi._opt(prev), n, w, h, h263mi._opt(change), cells,
                                             cells_bytes, summary, selected, count)


def test_the_structures_have_their_sizes():
    assert C.sizeof(h263mi.Change) == 16 and C.sizeof(h263mi.PlaneSet) == 32 and C.sizeof(h263mi.ChangeSummary) == 16
    assert h263mi.CHANGE_SUMMARY_DTYPE.itemsize == 16
    for name in ("h263mi_change_extent", "h263mi_change_map_on", "h263mi_batch_change_map", "h263mi_batch_change_last", "h263mi_change_last"):
        assert name in h263mi.EXPORTS and hasattr(h263mi.lib(), name)


def test_extent_values():
    assert h263mi.change_extent(3, 100, 60, h263mi.make_change(4)) == (7, 4, 3 * 7 * 4 * 4)
    assert h263mi.change_extent(1, 1, 1, h263mi.make_change(3)) == (1, 1, 4)
    assert h263mi.change_extent(0, 8, 8, h263mi.make_change(3)) == (1, 1, 0)
    assert h263mi.change_extent(2, 1025, 9, h263mi.make_change(3)) == (129, 2, 2 * 129 * 2 * 4)
    assert h263mi.change_extent(1, 1920, 1080, h263mi.make_change(4)) == (120, 68, 120 * 68 * 4)
    assert h263mi.change_extent(65535, 65535, 16383, h263mi.make_change(3)) == (8192, 2048, 65535 * 8192 * 2048 * 4)
    assert h263mi.change_extent(1, 64, 65, h263mi.make_change(6)) == (1, 2, 8)
    # the output pointers are optional
    assert h263mi.lib().h263mi_change_extent(1, 8, 8, C.byref(h263mi.make_change()), None, None, None) == OK


def test_extent_is_the_validator_of_the_description():
    ext = lambda n, w, h, c: h263mi.lib().h263mi_change_extent(n, w, h, h263mi._opt(c), None, None, None)
    assert ext(1, 8, 8, None) == BAD
    for cl in (0, 2, 7, 255):
        assert ext(1, 8, 8, h263mi.make_change(cl)) == BAD
    for cl in (3, 4, 5, 6):
        assert ext(1, 8, 8, h263mi.make_change(cl)) == OK
    assert ext(1, 8, 8, h263mi.make_change(roll=2)) == BAD
    assert ext(1, 8, 8, h263mi.make_change(roll=1)) == OK
    for k in range(2):
        c = h263mi.make_change()
        c.reserved[k] = 1
        assert ext(1, 8, 8, c) == BAD
    c = h263mi.make_change()
    c.reserved2 = 1
    assert ext(1, 8, 8, c) == BAD
    assert ext(1, 0, 8, h263mi.make_change()) == BAD and ext(1, 8, 0, h263mi.make_change()) == BAD
    assert ext(1, 65536, 1, h263mi.make_change()) == BAD and ext(1, 1, 65536, h263mi.make_change()) == BAD
    assert ext(1, 32768, 32768, h263mi.make_change()) == BAD
    assert ext(1, 32769, 32767, h263mi.make_change()) == OK
    assert ext(65536, 8, 8, h263mi.make_change()) == BAD and ext(65535, 8, 8, h263mi.make_change()) == OK


def test_refusals_of_the_call():
    # the description: a reserved byte, the cell, roll
    assert call(change=None) == BAD
    c = h263mi.make_change()
    c.reserved[1] = 7
    assert call(change=c) == BAD
    c = h263mi.make_change()
    c.reserved2 = 1 << 31
    assert call(change=c) == BAD
    assert call(change=h263mi.make_change(2)) == BAD and call(change=h263mi.make_change(7)) == BAD
    assert call(change=h263mi.make_change(roll=2)) == BAD
    # a zero size, a side above 65535, W*H >= 2^30
    assert call(w=0) == BAD and call(h=0) == BAD
    assert call(w=65536, h=1, n=1) == BAD
    assert call(w=32768, h=32768, n=1) == BAD
    assert call(w=32769, h=32767, n=1) == NO_DEVICE
    assert call(w=65535, h=1, n=1) == NO_DEVICE                     # not only decodable sizes
    # n_pictures > 65535
    assert call(n=65536, w=8, h=8) == BAD
    assert call(n=65535, w=8, h=8) == NO_DEVICE
    # a NULL that is needed
    assert call(cur=None) == BAD and call(prev=None) == BAD and call(summary=None) == BAD
    assert call(cur=plane_set(None)) == BAD and call(prev=plane_set(None)) == BAD
    assert call(cells=None, cells_bytes=0) == NO_DEVICE             # the grid is optional
    # pitch < W with H > 1
    assert call(cur=plane_set(CUR, pitch=W - 1, stride=H * W, nbytes=1 << 30)) == BAD
    assert call(prev=plane_set(PREV, pitch=W - 1, stride=H * W, nbytes=1 << 30)) == BAD
    assert call(h=1, cur=plane_set(CUR, h=1, pitch=0, stride=W), prev=plane_set(PREV, h=1, pitch=3, stride=W)) == NO_DEVICE
    # a set whose last byte lies behind `bytes`, computed without wrapping
    full = (N - 1) * H * W + (H - 1) * W + W
    assert call(cur=plane_set(CUR, nbytes=full - 1)) == BAD and call(prev=plane_set(PREV, nbytes=full - 1)) == BAD
    assert call(cur=plane_set(CUR, nbytes=full)) == NO_DEVICE
    assert call(cur=plane_set(CUR, stride=1 << 63, nbytes=(1 << 64) - 1)) == BAD               # (n-1) * stride wraps
    assert call(cur=plane_set(CUR, pitch=1 << 60, stride=0, nbytes=(1 << 64) - 1)) == BAD       # (H-1) * pitch wraps
    assert call(cur=plane_set(CUR, pitch=(1 << 64) // 59, stride=0, nbytes=(1 << 64) - 1)) == BAD      # the sum wraps
    # cells_bytes below the extent
    assert call(cells_bytes=N * 7 * 4 * 4 - 1) == BAD
    assert call(cells_bytes=N * 7 * 4 * 4) == NO_DEVICE
    # d_selected and d_count: both or neither
    assert call(selected=None) == BAD and call(count=None) == BAD
    assert call(selected=None, count=None) == NO_DEVICE


def test_cur_is_read_only_so_its_pictures_may_overlap():
    assert call(cur=plane_set(CUR, stride=0)) == NO_DEVICE
    assert call(cur=plane_set(CUR, stride=1)) == NO_DEVICE
    assert call(cur=plane_set(CUR, stride=0), change=h263mi.make_change(roll=1)) == NO_DEVICE
    # without roll prev is only read too
    assert call(prev=plane_set(PREV, stride=0)) == NO_DEVICE
    assert call(prev=plane_set(CUR)) == NO_DEVICE


def test_refusals_under_roll():
    roll = h263mi.make_change(roll=1)
    assert call(change=roll) == NO_DEVICE
    # prev pictures that overlap one another
    foot = (H - 1) * W + W
    assert call(change=roll, prev=plane_set(PREV, stride=foot - 1)) == BAD
    assert call(change=roll, prev=plane_set(PREV, stride=0)) == BAD
    assert call(change=roll, prev=plane_set(PREV, stride=foot)) == NO_DEVICE
    assert call(change=roll, n=1, prev=plane_set(PREV, n=1, stride=0)) == NO_DEVICE             # (one picture overlaps nothing)
    # prev's byte range intersecting cur's
    cur_bytes = (N - 1) * H * W + foot
    assert call(change=roll, prev=plane_set(CUR)) == BAD
    assert call(change=roll, prev=plane_set(CUR + cur_bytes - 1)) == BAD
    assert call(change=roll, prev=plane_set(CUR + cur_bytes)) == NO_DEVICE
    assert call(change=roll, prev=plane_set(CUR - cur_bytes + 1)) == BAD
    assert call(change=roll, prev=plane_set(CUR - cur_bytes)) == NO_DEVICE
    assert call(change=roll, cur=plane_set(CUR, stride=0), prev=plane_set(CUR + foot)) == NO_DEVICE    # (cur is one plane)


def test_an_earlier_refusal_wins_over_the_device_check_and_over_a_later_one():
    assert call(change=h263mi.make_change(9), cur=None, summary=None, n=70000, selected=None) == BAD


def test_no_pictures_is_ok_without_a_device_unless_a_count_is_wanted():
    assert call(n=0, selected=None, count=None) == OK
    assert call(n=0, cur=None, prev=None, cells=None, summary=None, selected=None, count=None) == OK
    assert call(n=0) == NO_DEVICE                                    # d_count still becomes 0: that takes a device
    # ... but the description and the pairing are still looked at
    assert call(n=0, change=None, selected=None, count=None) == BAD
    assert call(n=0, w=0, selected=None, count=None) == BAD
    assert call(n=0, count=None) == BAD


def test_the_batch_and_state_calls_refuse_no_handle():
    c, ps = h263mi.make_change(), plane_set()
    L = h263mi.lib()
    assert L.h263mi_batch_change_map(None, C.byref(ps), C.byref(ps), C.byref(c), CELLS, 1 << 20, SUMMARY, None, None) == BAD
    assert L.h263mi_batch_change_last(None, C.byref(ps), C.byref(c), CELLS, 1 << 20, SUMMARY, None, None, None) == BAD
    assert L.h263mi_change_last(None, C.byref(ps), C.byref(c), CELLS, 1 << 20, SUMMARY, None, None) == BAD


def test_a_valid_call_ends_at_the_device_check():
    assert call() == NO_DEVICE


@pytest.mark.skipif(not NO_GPU, reason="only meaningful where no GPU exists")
def test_a_valid_call_needs_a_device():
    c, cur, prev = h263mi.make_change(), plane_set(CUR), plane_set(PREV)
    assert h263mi.lib().h263mi_change_map_on(None, C.byref(cur), C.byref(prev), N, W, H, C.byref(c), CELLS, 1 << 20, SUMMARY, LIST,
                                             COUNT) == NO_DEVICE
    with pytest.raises(h263mi.H263Error) as e:
        h263mi.change_map(cur, prev, N, W, H, c, CELLS, 1 << 20, SUMMARY, LIST, COUNT)
    assert e.value.code == NO_DEVICE
