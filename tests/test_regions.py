"""CPU side of the motion regions (h263mi_regions_extent, h263mi_regions_on, h263mi_batch_regions): everything the host decides
before any device call -- the extents, every refusal include/h263mi.h lists, n_pictures == 0, and the device check behind them.  The
pointers are made-up addresses: nothing here dereferences them, and a call that passes the argument checks names a device that no
machine has, so that it ends at the device check wherever the suite runs."""
import ctypes as C
import os
import re

import pytest

import h263mi

BAD, OK, NO_DEVICE = h263mi.ERR_INVALID_ARGUMENT, h263mi.OK, h263mi.ERR_NO_DEVICE
NO_GPU = not os.path.exists("/dev/kfd")
NOWHERE = h263mi.BackendCfg(1 << 20, 0, None)                       # a device id beyond any machine's
CELLS, SUMMARY, WORK, ROIS, STATS, INFO, COUNT = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000
W, H, N, MAX_ROIS = 100, 60, 3, 40                                  # cell_log2 4: a grid of 7 x 4
DEFAULT = object()
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "h263mi.h")


def call(cells=CELLS, cells_bytes=None, summary=SUMMARY, n=N, w=W, h=H, regions=DEFAULT, work=WORK, work_bytes=None, rois=ROIS,
         max_rois=MAX_ROIS, stats=STATS, info=INFO, count=COUNT):
    regions = h263mi.make_regions() if regions is DEFAULT else regions
    ok = regions is not None and 3 <= regions.cell_log2 <= 6
    c = 1 << (regions.cell_log2 if ok else 4)
    if cells_bytes is None:
        cells_bytes = n * -(-w // c) * -(-h // c) * 4
    if work_bytes is None:
        work_bytes = n * (regions.max_per_picture if regions is not None else 16) * 32
    return h263mi.lib().h263mi_regions_on(C.byref(NOWHERE), cells, cells_bytes, summary, n, w, h, h263mi._opt(regions), work, work_bytes,
                                          rois, max_rois, stats, info, count)


def test_the_structures_have_their_sizes():
    assert C.sizeof(h263mi.Regions) == 16 and C.sizeof(h263mi.RegionInfo) == 16 and C.sizeof(h263mi.RegionStat) == 16
    assert C.sizeof(h263mi.Roi) == 16
    assert h263mi.REGION_INFO_DTYPE.itemsize == 16 and h263mi.REGION_STAT_DTYPE.itemsize == 16 and h263mi.ROI_DTYPE.itemsize == 16
    for name in ("h263mi_regions_extent", "h263mi_regions_on", "h263mi_batch_regions"):
        assert name in h263mi.EXPORTS and hasattr(h263mi.lib(), name)
    assert h263mi.lib().h263mi_abi_version() == 7


def _header_struct(name):
    """the fields of `typedef struct name { ... }` in include/h263mi.h as [(C type, field name)]"""
    text = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            out += [(ctype, f.strip()) for f in names.split(",")]
    return out


def test_the_python_structures_match_the_header():
    ctypes_of = {"uint8_t": C.c_uint8, "uint16_t": C.c_uint16, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
    for cname, cls in (("h263mi_regions", h263mi.Regions), ("h263mi_region_info", h263mi.RegionInfo), ("h263mi_region_stat", h263mi.RegionStat),
                       ("h263mi_roi", h263mi.Roi)):
        assert [(ctypes_of[t], f) for t, f in _header_struct(cname)] == [(t, f) for f, t in cls._fields_], cname
    for cls, dtype in ((h263mi.RegionInfo, h263mi.REGION_INFO_DTYPE), (h263mi.RegionStat, h263mi.REGION_STAT_DTYPE), (h263mi.Roi, h263mi.ROI_DTYPE)):
        assert [(f, getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_] == \
            [(f, dtype.fields[f][1], dtype.fields[f][0].itemsize) for f in dtype.names]
    assert "#define H263MI_REGIONS_MAX_CELLS 32768u" in open(HEADER).read() and h263mi.REGIONS_MAX_CELLS == 32768


def test_extent_values():
    r = h263mi.make_regions
    assert h263mi.regions_extent(3, 100, 60, r(4, max_per_picture=16)) == (7, 4, 3 * 7 * 4 * 4, 3 * 16 * 32)
    assert h263mi.regions_extent(1, 1, 1, r(3, max_per_picture=1)) == (1, 1, 4, 32)
    assert h263mi.regions_extent(0, 8, 8, r(3)) == (1, 1, 0, 0)
    assert h263mi.regions_extent(64, 1920, 1080, r(3, max_per_picture=256)) == (240, 135, 64 * 32400 * 4, 64 * 256 * 32)
    assert h263mi.regions_extent(1, 3840, 2160, r(4)) == (240, 135, 32400 * 4, 16 * 32)
    assert h263mi.regions_extent(65535, 2048, 1024, r(3, max_per_picture=256)) == (256, 128, 65535 * 32768 * 4, 65535 * 256 * 32)
    assert h263mi.regions_extent(1, 65535, 32, r(3)) == (8192, 4, 32768 * 4, 16 * 32)
    # the output pointers are optional
    assert h263mi.lib().h263mi_regions_extent(1, 8, 8, C.byref(r()), None, None, None, None) == OK


def test_extent_is_the_validator_of_the_description():
    ext = lambda n, w, h, r: h263mi.lib().h263mi_regions_extent(n, w, h, h263mi._opt(r), None, None, None, None)
    r = h263mi.make_regions
    assert ext(1, 8, 8, None) == BAD
    for cl in (0, 2, 7, 255):
        assert ext(1, 8, 8, r(cl)) == BAD
    for cl in (3, 4, 5, 6):
        assert ext(1, 8, 8, r(cl)) == OK
    for conn in (0, 1, 5, 6, 12, 255):
        assert ext(1, 8, 8, r(connectivity=conn)) == BAD
    assert ext(1, 8, 8, r(connectivity=4)) == OK and ext(1, 8, 8, r(connectivity=8)) == OK
    assert ext(1, 8, 8, r(margin_cells=9)) == BAD and ext(1, 8, 8, r(margin_cells=8)) == OK and ext(1, 8, 8, r(margin_cells=0)) == OK
    assert ext(1, 8, 8, r(min_cells=0)) == BAD and ext(1, 8, 8, r(min_cells=0xFFFFFFFF)) == OK
    assert ext(1, 8, 8, r(max_per_picture=0)) == BAD and ext(1, 8, 8, r(max_per_picture=257)) == BAD
    assert ext(1, 8, 8, r(max_per_picture=1)) == OK and ext(1, 8, 8, r(max_per_picture=256)) == OK
    d = r()
    d.reserved = 1
    assert ext(1, 8, 8, d) == BAD
    assert ext(1, 0, 8, r()) == BAD and ext(1, 8, 0, r()) == BAD
    assert ext(1, 65536, 1, r()) == BAD and ext(1, 1, 65536, r()) == BAD
    assert ext(1, 32768, 32768, r(6)) == BAD                       # W*H >= 2^30
    assert ext(65536, 8, 8, r()) == BAD and ext(65535, 8, 8, r()) == OK
    # the cap: gw*gh <= 32768
    assert ext(1, 2048, 1024, r(3)) == OK and ext(1, 2049, 1024, r(3)) == BAD and ext(1, 2048, 1025, r(3)) == BAD
    assert ext(1, 1920, 1080, r(3)) == OK and ext(1, 3840, 2160, r(3)) == BAD and ext(1, 3840, 2160, r(4)) == OK
    assert ext(1, 65535, 32, r(3)) == OK and ext(1, 65535, 33, r(3)) == BAD


def test_refusals_of_the_call():
    r = h263mi.make_regions
    assert call() == NO_DEVICE
    # anything the extent call refuses, a grid above the cap included
    assert call(regions=None) == BAD
    assert call(regions=r(2)) == BAD and call(regions=r(connectivity=6)) == BAD and call(regions=r(margin_cells=9)) == BAD
    assert call(regions=r(min_cells=0)) == BAD and call(regions=r(max_per_picture=257)) == BAD
    assert call(w=0) == BAD and call(h=0) == BAD and call(w=65536, h=1) == BAD and call(n=65536, w=8, h=8) == BAD
    assert call(w=2049, h=1024, regions=r(3), n=1) == BAD and call(w=2048, h=1024, regions=r(3), n=1) == NO_DEVICE
    # a NULL that is needed
    assert call(cells=None) == BAD and call(work=None) == BAD and call(rois=None) == BAD and call(info=None) == BAD and call(count=None) == BAD
    assert call(stats=None) == NO_DEVICE and call(summary=None) == NO_DEVICE              # both are optional
    # a byte count below its extent
    assert call(cells_bytes=N * 7 * 4 * 4 - 1) == BAD and call(cells_bytes=N * 7 * 4 * 4) == NO_DEVICE
    assert call(work_bytes=N * 16 * 32 - 1) == BAD and call(work_bytes=N * 16 * 32) == NO_DEVICE
    assert call(regions=r(max_per_picture=256), work_bytes=N * 256 * 32 - 1) == BAD
    # max_rois
    assert call(max_rois=0) == BAD and call(max_rois=65536) == BAD
    assert call(max_rois=1) == NO_DEVICE and call(max_rois=65535) == NO_DEVICE
    # alignment: 4, 8, 8, 4, 4 bytes for cells, work, stats, info, count; 4 for rois; 8 for the summaries
    for k in (1, 2, 3):
        assert call(cells=CELLS + k) == BAD and call(rois=ROIS + k) == BAD and call(info=INFO + k) == BAD and call(count=COUNT + k) == BAD
    for k in (1, 2, 4, 7):
        assert call(work=WORK + k) == BAD and call(stats=STATS + k) == BAD and call(summary=SUMMARY + k) == BAD
    assert call(cells=CELLS + 4) == NO_DEVICE and call(rois=ROIS + 4) == NO_DEVICE and call(info=INFO + 4) == NO_DEVICE
    assert call(count=COUNT + 4) == NO_DEVICE and call(work=WORK + 8) == NO_DEVICE and call(stats=STATS + 8) == NO_DEVICE


def test_an_output_may_not_intersect_an_input_or_another_output():
    cells_bytes, work_bytes, table = N * 7 * 4 * 4, N * 16 * 32, MAX_ROIS * 16
    sizes = {"cells": cells_bytes, "summary": N * 16, "work": work_bytes, "rois": table, "stats": table, "info": N * 16, "count": 8}
    outputs = ("work", "rois", "stats", "info", "count")
    for out in outputs:
        for other in sizes:
            if other == out:
                continue
            base = 0x900000
            # `out` begins inside `other`'s last 8 bytes; then right behind it
            assert call(**{other: base, out: base + sizes[other] - 8}) == BAD, (out, other)
            assert call(**{other: base, out: base + sizes[other]}) == NO_DEVICE, (out, other)
            # `other` begins inside `out`'s last 8 bytes
            assert call(**{out: base, other: base + sizes[out] - 8}) == BAD, (out, other)
    # the two inputs may share their bytes: both are only read
    assert call(cells=0x900000, summary=0x900000) == NO_DEVICE


def test_an_earlier_refusal_wins_over_the_device_check_and_over_a_later_one():
    assert call(regions=h263mi.make_regions(9), cells=None, n=70000, max_rois=0) == BAD


def test_no_pictures_still_takes_a_device_for_the_table():
    assert call(n=0) == NO_DEVICE                                    # the table is filled, the counts become 0
    assert call(n=0, cells=None, work=None, info=None, summary=None, stats=None, cells_bytes=0, work_bytes=0) == NO_DEVICE
    assert call(n=0, rois=None) == BAD and call(n=0, count=None) == BAD and call(n=0, max_rois=0) == BAD
    assert call(n=0, regions=None) == BAD and call(n=0, w=0) == BAD


def test_the_batch_call_refuses_no_handle():
    r = h263mi.make_regions()
    assert h263mi.lib().h263mi_batch_regions(None, CELLS, 1 << 20, None, C.byref(r), WORK, 1 << 20, ROIS, MAX_ROIS, None, INFO, COUNT) == BAD


@pytest.mark.skipif(not NO_GPU, reason="only meaningful where no GPU exists")
def test_a_valid_call_needs_a_device():
    r = h263mi.make_regions()
    assert h263mi.lib().h263mi_regions_on(None, CELLS, 1 << 20, None, N, W, H, C.byref(r), WORK, 1 << 20, ROIS, MAX_ROIS, None, INFO,
                                          COUNT) == NO_DEVICE
    with pytest.raises(h263mi.H263Error) as e:
        h263mi.regions(CELLS, 1 << 20, N, W, H, r, WORK, 1 << 20, ROIS, MAX_ROIS, INFO, COUNT)
    assert e.value.code == NO_DEVICE
