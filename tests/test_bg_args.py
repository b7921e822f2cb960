"""CPU side of the background model (h263mi_background_extent, h263mi_background_on, h263mi_batch_background,
h263mi_batch_background_last, h263mi_background_last): everything the host decides before any device call -- the extents, every
refusal include/h263mi.h lists, n_pictures == 0, and the device check behind them.  The pointers are made-up addresses: nothing here
dereferences them, and a call that passes the argument checks names a device that no machine has, so that it ends at the device
check wherever the suite runs."""
import ctypes as C
import os

import pytest

import h263mi

BAD, OK, NO_DEVICE = h263mi.ERR_INVALID_ARGUMENT, h263mi.OK, h263mi.ERR_NO_DEVICE
NO_GPU = not os.path.exists("/dev/kfd")
NOWHERE = h263mi.BackendCfg(1 << 20, 0, None)                       # a device id beyond any machine's
CUR, STATE, MASK, CELLS, SUMMARY, LIST, COUNT, CUT, CUT_COUNT = (k << 40 for k in range(1, 10))      # (a terabyte apart)
W, H, N = 100, 60, 3
STRIDE = 64 + H * 32 * 7                                            # ceil(100 / 16) = 7 chunks a row
DEFAULT = object()


def plane_set(base=CUR, w=W, h=H, n=N, pitch=None, stride=None, nbytes=None):
    pitch = w if pitch is None else pitch
    stride = h * pitch if stride is None else stride
    nbytes = (n - 1) * stride + (h - 1) * pitch + w if nbytes is None else nbytes
    return h263mi.PlaneSet(base, nbytes, pitch, stride)


def call(cur=DEFAULT, n=N, w=W, h=H, bg=DEFAULT, state=STATE, state_bytes=None, cut=CUT, cut_count=CUT_COUNT, mask=DEFAULT, cells=CELLS,
         cells_bytes=None, summary=SUMMARY, selected=LIST, count=COUNT):
    cur = plane_set(CUR, w, h, max(n, 1)) if cur is DEFAULT else cur
    mask = plane_set(MASK, w, h, max(n, 1)) if mask is DEFAULT else mask
    bg = h263mi.make_background() if bg is DEFAULT else bg
    cl = bg.cell_log2 if bg is not None and 3 <= bg.cell_log2 <= 6 else 4
    if cells_bytes is None:
        cells_bytes = n * -(-w // (1 << cl)) * -(-h // (1 << cl)) * 4
    if state_bytes is None:
        state_bytes = n * (64 + h * 32 * -(-w // 16))
    return h263mi.lib().h263mi_background_on(C.byref(NOWHERE), h263mi._opt(cur), n, w, h, h263mi._opt(bg), state, state_bytes, cut, cut_count,
                                             h263mi._opt(mask), cells, cells_bytes, summary, selected, count)


def test_the_structures_have_their_sizes():
    assert C.sizeof(h263mi.Background) == 16 and C.sizeof(h263mi.BackgroundHead) == 64 and h263mi.BACKGROUND_HEAD_DTYPE.itemsize == 64
    assert h263mi.Background.warmup.offset == 4 and h263mi.Background.cell_threshold.offset == 8
    assert h263mi.Background.min_changed_cells.offset == 12 and h263mi.Background.pixel_threshold.offset == 3
    for name in ("h263mi_background_extent", "h263mi_background_on", "h263mi_batch_background", "h263mi_batch_background_last",
                 "h263mi_background_last"):
        assert name in h263mi.EXPORTS and hasattr(h263mi.lib(), name)
    assert h263mi.lib().h263mi_abi_version() == 7


def test_extent_values():
    ext = h263mi.background_extent
    assert ext(3, 100, 60, h263mi.make_background(4)) == (7, 4, 3 * 7 * 4 * 4, 3 * STRIDE)
    assert ext(1, 1, 1, h263mi.make_background(3)) == (1, 1, 4, 64 + 32)
    assert ext(0, 8, 8, h263mi.make_background(3)) == (1, 1, 0, 0)
    assert ext(1, 16, 2, h263mi.make_background(3)) == (2, 1, 8, 64 + 2 * 32)
    assert ext(1, 17, 2, h263mi.make_background(3)) == (3, 1, 12, 64 + 2 * 64)
    assert ext(2, 1025, 9, h263mi.make_background(3)) == (129, 2, 2 * 129 * 2 * 4, 2 * (64 + 9 * 32 * 65))
    assert ext(64, 1920, 1080, h263mi.make_background(4)) == (120, 68, 64 * 120 * 68 * 4, 64 * (64 + 1080 * 3840))
    assert ext(65535, 65535, 16383, h263mi.make_background(3)) == (8192, 2048, 65535 * 8192 * 2048 * 4, 65535 * (64 + 16383 * 32 * 4096))
    # the output pointers are optional
    assert h263mi.lib().h263mi_background_extent(1, 8, 8, C.byref(h263mi.make_background()), None, None, None, None) == OK


def test_extent_is_the_validator_of_the_description():
    ext = lambda n, w, h, b: h263mi.lib().h263mi_background_extent(n, w, h, h263mi._opt(b), None, None, None, None)
    mk = h263mi.make_background
    assert ext(1, 8, 8, None) == BAD
    for cl in (0, 2, 7, 255):
        assert ext(1, 8, 8, mk(cl)) == BAD
    for cl in (3, 4, 5, 6):
        assert ext(1, 8, 8, mk(cl)) == OK
    for s in range(8):
        assert ext(1, 8, 8, mk(learn_shift=s, fg_learn_shift=s)) == OK
    assert ext(1, 8, 8, mk(learn_shift=8)) == BAD and ext(1, 8, 8, mk(learn_shift=255)) == BAD
    assert ext(1, 8, 8, mk(fg_learn_shift=8)) == BAD and ext(1, 8, 8, mk(fg_learn_shift=254)) == BAD
    assert ext(1, 8, 8, mk(fg_learn_shift=255)) == OK
    assert ext(1, 8, 8, mk(pixel_threshold=0, warmup=65535, cell_threshold=0xFFFFFFFF, min_changed_cells=0xFFFFFFFF)) == OK
    assert ext(1, 8, 8, mk(pixel_threshold=255)) == OK
    b = mk()
    b.reserved = 1
    assert ext(1, 8, 8, b) == BAD
    assert ext(1, 0, 8, mk()) == BAD and ext(1, 8, 0, mk()) == BAD
    assert ext(1, 65536, 1, mk()) == BAD and ext(1, 1, 65536, mk()) == BAD
    assert ext(1, 32768, 32768, mk()) == BAD and ext(1, 32769, 32767, mk()) == OK
    assert ext(65536, 8, 8, mk()) == BAD and ext(65535, 8, 8, mk()) == OK


def test_refusals_of_the_call():
    mk = h263mi.make_background
    # anything the extent call refuses
    assert call(bg=None) == BAD
    b = mk()
    b.reserved = 0x8000
    assert call(bg=b) == BAD
    assert call(bg=mk(2)) == BAD and call(bg=mk(7)) == BAD and call(bg=mk(learn_shift=8)) == BAD and call(bg=mk(fg_learn_shift=100)) == BAD
    assert call(w=0) == BAD and call(h=0) == BAD and call(w=65536, h=1, n=1) == BAD and call(w=32768, h=32768, n=1) == BAD
    assert call(w=32769, h=32767, n=1) == NO_DEVICE and call(w=65535, h=1, n=1) == NO_DEVICE
    assert call(n=65536, w=8, h=8) == BAD and call(n=65535, w=8, h=8) == NO_DEVICE
    # NULL required pointers while n > 0
    assert call(cur=None) == BAD and call(state=None) == BAD and call(summary=None) == BAD
    assert call(cur=plane_set(None)) == BAD and call(mask=plane_set(None)) == BAD
    assert call(cells=None, cells_bytes=0) == NO_DEVICE and call(mask=None) == NO_DEVICE          # the grid and the mask are optional
    # pitch < W with H > 1
    assert call(cur=plane_set(CUR, pitch=W - 1, stride=H * W, nbytes=1 << 20)) == BAD
    assert call(mask=plane_set(MASK, pitch=W - 1, stride=H * W, nbytes=1 << 20)) == BAD
    assert call(h=1, cur=plane_set(CUR, h=1, pitch=0, stride=W), mask=plane_set(MASK, h=1, pitch=3, stride=W)) == NO_DEVICE
    # a set or a buffer shorter than its extent, computed without wrapping
    full = (N - 1) * H * W + (H - 1) * W + W
    assert call(cur=plane_set(CUR, nbytes=full - 1)) == BAD and call(mask=plane_set(MASK, nbytes=full - 1)) == BAD
    assert call(cur=plane_set(CUR, nbytes=full)) == NO_DEVICE
    assert call(cur=plane_set(CUR, stride=1 << 63, nbytes=(1 << 64) - 1)) == BAD               # (n-1) * stride wraps
    assert call(cur=plane_set(CUR, pitch=1 << 60, stride=0, nbytes=(1 << 64) - 1)) == BAD       # (H-1) * pitch wraps
    assert call(cur=plane_set(CUR, pitch=(1 << 64) // 59, stride=0, nbytes=(1 << 64) - 1)) == BAD      # the sum wraps
    assert call(n=1, mask=plane_set(MASK, n=1, pitch=1 << 60, stride=0, nbytes=(1 << 64) - 1)) == BAD
    assert call(state_bytes=N * STRIDE - 1) == BAD and call(state_bytes=N * STRIDE) == NO_DEVICE
    assert call(cells_bytes=N * 7 * 4 * 4 - 1) == BAD and call(cells_bytes=N * 7 * 4 * 4) == NO_DEVICE
    # d_state not a multiple of 32
    for off in (1, 4, 8, 16, 48):
        assert call(state=STATE + off) == BAD
    assert call(state=STATE + 32) == NO_DEVICE
    # d_cut and d_cut_count, d_selected and d_count: both or neither
    assert call(cut=None) == BAD and call(cut_count=None) == BAD and call(cut=None, cut_count=None) == NO_DEVICE
    assert call(selected=None) == BAD and call(count=None) == BAD and call(selected=None, count=None) == NO_DEVICE
    # overlapping pictures in the mask
    foot = (H - 1) * W + W
    assert call(mask=plane_set(MASK, stride=foot - 1)) == BAD and call(mask=plane_set(MASK, stride=0)) == BAD
    assert call(mask=plane_set(MASK, stride=foot)) == NO_DEVICE
    assert call(n=1, mask=plane_set(MASK, n=1, stride=0)) == NO_DEVICE                         # (one picture overlaps nothing)


def test_cur_is_read_only_so_its_pictures_may_overlap():
    assert call(cur=plane_set(CUR, stride=0)) == NO_DEVICE and call(cur=plane_set(CUR, stride=1)) == NO_DEVICE


def test_an_output_may_not_intersect_an_input_or_another_output():
    full = (N - 1) * H * W + (H - 1) * W + W
    extent = {"state": N * STRIDE, "mask": full, "cells": N * 7 * 4 * 4, "summary": N * 16, "selected": N * 4, "count": 4, "cur": full,
              "cut": N * 4, "cut_count": 4}
    base = {"state": STATE, "mask": MASK, "cells": CELLS, "summary": SUMMARY, "selected": LIST, "count": COUNT, "cur": CUR, "cut": CUT,
            "cut_count": CUT_COUNT}

    def at(name, addr):
        if name in ("mask", "cur"):
            return {name: plane_set(addr)}
        return {name: addr}
    outputs = ["state", "mask", "cells", "summary", "selected", "count"]
    for i, out in enumerate(outputs):
        for other in outputs[i + 1:] + ["cur", "cut", "cut_count"]:
            # `out` moved to end one byte inside `other`, then to just behind it (the state in steps of 32)
            step = 32 if out == "state" else 1
            last = base[other] + extent[other] - 1
            inside = last - last % step
            behind = -(-(base[other] + extent[other]) // step) * step
            assert call(**at(out, inside)) == BAD, (out, other)
            assert call(**at(out, behind)) == NO_DEVICE, (out, other)
            # ... and `out` ending one byte inside `other`
            if out != "state":
                assert call(**at(out, base[other] - extent[out] + 1)) == BAD, (out, other)
                assert call(**at(out, base[other] - extent[out])) == NO_DEVICE, (out, other)
    # the inputs may share bytes with one another
    assert call(cut=CUR, cut_count=CUR) == NO_DEVICE
    # an absent output intersects nothing
    assert call(cells=None, cells_bytes=0, mask=None, selected=None, count=None) == NO_DEVICE


def test_an_earlier_refusal_wins_over_the_device_check_and_over_a_later_one():
    assert call(bg=h263mi.make_background(9), cur=None, summary=None, n=70000, selected=None, state=STATE + 1) == BAD


def test_no_pictures_is_ok_without_a_device_unless_a_count_is_wanted():
    assert call(n=0, selected=None, count=None) == OK
    assert call(n=0, cur=None, state=None, mask=None, cells=None, summary=None, selected=None, count=None, cut=None, cut_count=None) == OK
    assert call(n=0) == NO_DEVICE                                    # d_count still becomes 0: that takes a device
    # ... but the description and the pairings are still looked at
    assert call(n=0, bg=None, selected=None, count=None) == BAD
    assert call(n=0, w=0, selected=None, count=None) == BAD
    assert call(n=0, count=None) == BAD and call(n=0, cut=None, selected=None, count=None) == BAD


def test_the_batch_and_state_calls_refuse_no_handle():
    b, ps = h263mi.make_background(), plane_set()
    L = h263mi.lib()
    assert L.h263mi_batch_background(None, C.byref(ps), C.byref(b), STATE, 1 << 30, None, None, None, CELLS, 1 << 20, SUMMARY, None, None) == BAD
    assert L.h263mi_batch_background_last(None, C.byref(b), STATE, 1 << 30, None, None, None, CELLS, 1 << 20, SUMMARY, None, None, None) == BAD
    assert L.h263mi_background_last(None, C.byref(b), STATE, 1 << 30, None, None, None, CELLS, 1 << 20, SUMMARY, None, None) == BAD


def test_a_valid_call_ends_at_the_device_check():
    assert call() == NO_DEVICE


@pytest.mark.skipif(not NO_GPU, reason="only meaningful where no GPU exists")
def test_a_valid_call_needs_a_device():
    with pytest.raises(h263mi.H263Error) as e:
        h263mi.background_on(plane_set(CUR), N, W, H, h263mi.make_background(), STATE, N * STRIDE, CELLS, 1 << 20, SUMMARY, LIST, COUNT)
    assert e.value.code == NO_DEVICE
