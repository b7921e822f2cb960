"""CPU side of the plane histograms (h263mi_hist_extent, h263mi_hist_on, h263mi_batch_hist, h263mi_batch_hist_last,
h263mi_hist_last): everything the host decides before any device call -- the extent, every refusal include/h263mi.h lists,
n_pictures == 0, and the device check behind them.  The pointers are made-up addresses: nothing here dereferences them, and a call
that passes the argument checks names a device that no machine has, so that it ends at the device check wherever the suite runs."""
import ctypes as C
import os

import pytest

import h263mi

BAD, OK, NO_DEVICE = h263mi.ERR_INVALID_ARGUMENT, h263mi.OK, h263mi.ERR_NO_DEVICE
NO_GPU = not os.path.exists("/dev/kfd")
NOWHERE = h263mi.BackendCfg(1 << 20, 0, None)                       # a device id beyond any machine's
SET, HIST, PREV, STATS, LIST, COUNT = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000
W, H, N = 100, 60, 3
DEFAULT = object()


def plane_set(base=SET, w=W, h=H, n=N, pitch=None, stride=None, nbytes=None):
    pitch = w if pitch is None else pitch
    stride = h * pitch if stride is None else stride
    nbytes = (n - 1) * stride + (h - 1) * pitch + w if nbytes is None else nbytes
    return h263mi.PlaneSet(base, nbytes, pitch, stride)


def call(pset=DEFAULT, n=N, w=W, h=H, hist=DEFAULT, d_hist=HIST, hist_bytes=None, prev=PREV, prev_bytes=None, stats=STATS, selected=LIST,
         count=COUNT):
    pset = plane_set(SET, w, h, max(n, 1)) if pset is DEFAULT else pset
    hist = h263mi.make_hist() if hist is DEFAULT else hist
    hist_bytes = n * 1024 if hist_bytes is None else hist_bytes
    prev_bytes = n * 1024 if prev_bytes is None else prev_bytes
    return h263mi.lib().h263mi_hist_on(C.byref(NOWHERE), h263mi._opt(pset), n, w, h, h263mi._opt(hist), d_hist, hist_bytes, prev, prev_bytes,
                                       stats, selected, count)


def test_the_structures_have_their_sizes():
    assert C.sizeof(h263mi.Hist) == 16 and C.sizeof(h263mi.HistStats) == 32 and h263mi.HIST_STATS_DTYPE.itemsize == 32
    assert [h263mi.HIST_STATS_DTYPE.fields[k][1] for k in ("sum", "sum_sq", "distance", "min", "max", "p_lo", "p_hi", "mode", "reserved")] == \
        [0, 8, 16, 24, 25, 26, 27, 28, 29]
    assert [getattr(h263mi.HistStats, k).offset for k in ("sum", "sum_sq", "distance", "min", "max", "p_lo", "p_hi", "mode", "reserved")] == \
        [0, 8, 16, 24, 25, 26, 27, 28, 29]
    assert [getattr(h263mi.Hist, k).offset for k in ("roll", "reserved", "lo_permille", "hi_permille", "cut_permille", "reserved2")] == \
        [0, 1, 4, 6, 8, 12]
    for name in ("h263mi_hist_extent", "h263mi_hist_on", "h263mi_batch_hist", "h263mi_batch_hist_last", "h263mi_hist_last"):
        assert name in h263mi.EXPORTS and hasattr(h263mi.lib(), name)
    assert h263mi.lib().h263mi_abi_version() == 7                   # additive


def test_extent_values():
    d = h263mi.make_hist()
    assert h263mi.hist_extent(3, 100, 60, d) == 3 * 1024
    assert h263mi.hist_extent(1, 1, 1, d) == 1024
    assert h263mi.hist_extent(0, 8, 8, d) == 0
    assert h263mi.hist_extent(64, 1920, 1080, d) == 65536
    assert h263mi.hist_extent(65535, 65535, 16383, d) == 65535 * 1024
    # the output pointer is optional
    assert h263mi.lib().h263mi_hist_extent(1, 8, 8, C.byref(d), None) == OK


def test_extent_is_the_validator_of_the_description():
    ext = lambda n, w, h, d: h263mi.lib().h263mi_hist_extent(n, w, h, h263mi._opt(d), None)
    assert ext(1, 8, 8, None) == BAD
    assert ext(1, 8, 8, h263mi.make_hist()) == OK
    for k in range(3):
        d = h263mi.make_hist()
        d.reserved[k] = 1
        assert ext(1, 8, 8, d) == BAD
    d = h263mi.make_hist()
    d.reserved2 = 1
    assert ext(1, 8, 8, d) == BAD
    assert ext(1, 8, 8, h263mi.make_hist(roll=2)) == BAD and ext(1, 8, 8, h263mi.make_hist(roll=1)) == OK
    # a permille above 1000, each of the three; lo > hi
    assert ext(1, 8, 8, h263mi.make_hist(0, 1000, 1000)) == OK
    assert ext(1, 8, 8, h263mi.make_hist(0, 1001, 0)) == BAD
    assert ext(1, 8, 8, h263mi.make_hist(1001, 1001, 0)) == BAD
    assert ext(1, 8, 8, h263mi.make_hist(0, 1000, 1001)) == BAD
    assert ext(1, 8, 8, h263mi.make_hist(501, 500)) == BAD and ext(1, 8, 8, h263mi.make_hist(500, 500)) == OK
    assert ext(1, 8, 8, h263mi.make_hist(1000, 1000)) == OK and ext(1, 8, 8, h263mi.make_hist(0, 0)) == OK
    # the size and the count
    assert ext(1, 0, 8, h263mi.make_hist()) == BAD and ext(1, 8, 0, h263mi.make_hist()) == BAD
    assert ext(1, 65536, 1, h263mi.make_hist()) == BAD and ext(1, 1, 65536, h263mi.make_hist()) == BAD
    assert ext(1, 65535, 1, h263mi.make_hist()) == OK and ext(1, 1, 65535, h263mi.make_hist()) == OK
    assert ext(1, 32768, 32768, h263mi.make_hist()) == BAD
    assert ext(1, 32769, 32767, h263mi.make_hist()) == OK
    assert ext(65536, 8, 8, h263mi.make_hist()) == BAD and ext(65535, 8, 8, h263mi.make_hist()) == OK


def test_refusals_of_the_call():
    # what the extent refuses
    assert call(hist=None) == BAD
    d = h263mi.make_hist()
    d.reserved[2] = 7
    assert call(hist=d) == BAD
    d = h263mi.make_hist()
    d.reserved2 = 1 << 31
    assert call(hist=d) == BAD
    assert call(hist=h263mi.make_hist(roll=2)) == BAD and call(hist=h263mi.make_hist(roll=1)) == NO_DEVICE
    assert call(hist=h263mi.make_hist(hi_permille=1001)) == BAD and call(hist=h263mi.make_hist(hi_permille=1000)) == NO_DEVICE
    assert call(hist=h263mi.make_hist(cut_permille=1001)) == BAD and call(hist=h263mi.make_hist(cut_permille=1000)) == NO_DEVICE
    assert call(hist=h263mi.make_hist(600, 599)) == BAD and call(hist=h263mi.make_hist(600, 600)) == NO_DEVICE
    assert call(w=0) == BAD and call(h=0) == BAD
    assert call(w=65536, h=1, n=1) == BAD and call(w=65535, h=1, n=1) == NO_DEVICE
    assert call(w=32768, h=32768, n=1) == BAD and call(w=32769, h=32767, n=1) == NO_DEVICE
    assert call(n=65536, w=8, h=8, prev=1 << 40) == BAD and call(n=65535, w=8, h=8, prev=1 << 40) == NO_DEVICE     # (64 MiB of histograms)
    # a NULL that is needed
    assert call(pset=None) == BAD and call(d_hist=None) == BAD and call(stats=None) == BAD and call(pset=plane_set(None)) == BAD
    # pitch < W with H > 1
    assert call(pset=plane_set(SET, pitch=W - 1, stride=H * W, nbytes=1 << 30)) == BAD
    assert call(pset=plane_set(SET, pitch=W, stride=H * W, nbytes=1 << 30)) == NO_DEVICE
    assert call(h=1, pset=plane_set(SET, h=1, pitch=0, stride=W)) == NO_DEVICE
    # a set whose last byte lies behind `bytes`, computed without wrapping
    full = (N - 1) * H * W + (H - 1) * W + W
    assert call(pset=plane_set(SET, nbytes=full - 1)) == BAD and call(pset=plane_set(SET, nbytes=full)) == NO_DEVICE
    assert call(pset=plane_set(SET, stride=1 << 63, nbytes=(1 << 64) - 1)) == BAD               # (n-1) * stride wraps
    assert call(pset=plane_set(SET, pitch=1 << 60, stride=0, nbytes=(1 << 64) - 1)) == BAD       # (H-1) * pitch wraps
    assert call(pset=plane_set(SET, pitch=(1 << 64) // 59, stride=0, nbytes=(1 << 64) - 1)) == BAD      # the sum wraps
    # hist_bytes or prev_bytes below the extent
    assert call(hist_bytes=N * 1024 - 1) == BAD and call(hist_bytes=N * 1024) == NO_DEVICE
    assert call(prev_bytes=N * 1024 - 1) == BAD and call(prev_bytes=N * 1024) == NO_DEVICE
    assert call(prev=None, prev_bytes=0, selected=None, count=None) == NO_DEVICE                # (no prev: its bytes do not count)
    # alignment: 4, 4 and 8
    for off in (1, 2, 3):
        assert call(d_hist=HIST + off) == BAD and call(prev=PREV + off) == BAD
    assert call(d_hist=HIST + 4) == NO_DEVICE and call(prev=PREV + 4) == NO_DEVICE
    for off in (1, 2, 4, 7):
        assert call(stats=STATS + off) == BAD
    assert call(stats=STATS + 8) == NO_DEVICE
    # prev's range intersecting the histograms'
    ext = N * 1024
    assert call(prev=HIST) == BAD
    assert call(prev=HIST + ext - 4) == BAD and call(prev=HIST + ext) == NO_DEVICE
    assert call(prev=HIST - ext + 4) == BAD and call(prev=HIST - ext) == NO_DEVICE
    # roll or a list without prev
    assert call(prev=None, selected=None, count=None, hist=h263mi.make_hist(roll=1)) == BAD
    assert call(prev=None) == BAD
    assert call(prev=None, selected=None, count=None) == NO_DEVICE
    # d_selected and d_count: both or neither
    assert call(selected=None) == BAD and call(count=None) == BAD
    assert call(selected=None, count=None) == NO_DEVICE


def test_the_set_is_read_only_so_its_pictures_may_overlap():
    assert call(pset=plane_set(SET, stride=0)) == NO_DEVICE
    assert call(pset=plane_set(SET, stride=1)) == NO_DEVICE
    assert call(pset=plane_set(SET, stride=0), hist=h263mi.make_hist(roll=1)) == NO_DEVICE
    assert call(pset=plane_set(SET + 1, pitch=W + 1)) == NO_DEVICE            # any alignment


def test_an_earlier_refusal_wins_over_the_device_check_and_over_a_later_one():
    assert call(hist=h263mi.make_hist(roll=9), pset=None, stats=None, n=70000, selected=None) == BAD


def test_no_pictures_is_ok_without_a_device_unless_a_count_is_wanted():
    assert call(n=0, selected=None, count=None) == OK
    assert call(n=0, pset=None, d_hist=None, prev=None, stats=None, selected=None, count=None) == OK
    assert call(n=0) == NO_DEVICE                                    # d_count still becomes 0: that takes a device
    # ... but the description and the pairing are still looked at
    assert call(n=0, hist=None, selected=None, count=None) == BAD
    assert call(n=0, w=0, selected=None, count=None) == BAD
    assert call(n=0, count=None) == BAD
    assert call(n=0, prev=None) == BAD


def test_the_batch_and_state_calls_refuse_no_handle():
    d, ps = h263mi.make_hist(), plane_set()
    L = h263mi.lib()
    assert L.h263mi_batch_hist(None, C.byref(ps), C.byref(d), HIST, 1 << 20, None, 0, STATS, None, None) == BAD
    assert L.h263mi_batch_hist_last(None, 0, C.byref(d), HIST, 1 << 20, None, 0, STATS, None, None, None) == BAD
    assert L.h263mi_hist_last(None, 0, C.byref(d), HIST, 1 << 20, None, 0, STATS, None, None) == BAD


def test_a_valid_call_ends_at_the_device_check():
    assert call() == NO_DEVICE


@pytest.mark.skipif(not NO_GPU, reason="only meaningful where no GPU exists")
def test_a_valid_call_needs_a_device():
    d, ps = h263mi.make_hist(), plane_set()
    assert h263mi.lib().h263mi_hist_on(None, C.byref(ps), N, W, H, C.byref(d), HIST, N * 1024, PREV, N * 1024, STATS, LIST, COUNT) == NO_DEVICE
    with pytest.raises(h263mi.H263Error) as e:
        h263mi.hist(ps, N, W, H, d, HIST, N * 1024, STATS, PREV, N * 1024, LIST, COUNT)
    assert e.value.code == NO_DEVICE
