"""h263mi_yuv_layout_extent (include/h263mi.h): a pure host function -- the bytes a layout of the deblocked planes needs and
every refusal, against values derived by hand here.  No device."""
import ctypes as C

import numpy as np
import pytest

import h263mi

I420, NV12 = h263mi.YUV_I420, h263mi.YUV_NV12


def extent(n, w, h, **kw):
    return h263mi.yuv_layout_extent(n, w, h, **kw)


def refused(n, w, h, **kw):
    with pytest.raises(h263mi.H263Error) as e:
        h263mi.yuv_layout_extent(n, w, h, **kw)
    return e.value.code == h263mi.ERR_INVALID_ARGUMENT


def test_the_null_layout_is_tightly_packed_i420():
    for n, w, h in ((1, 176, 144), (64, 1920, 1080), (3, 7, 9), (2, 1, 1)):
        cw, ch = (w + 1) // 2, (h + 1) // 2
        assert extent(n, w, h, default=True) == n * (w * h + 2 * cw * ch)
        # ... and so is I420 with both pitches 0
        assert extent(n, w, h, format=I420) == n * (w * h + 2 * cw * ch)


def test_extents_of_default_placement():
    # 1920 x 1080 NV12, both pitches 2048: 1080 luma rows and 540 rows of Cb,Cr pairs per picture
    assert extent(1, 1920, 1080, format=NV12, pitch_y=2048, pitch_c=2048) == 1080 * 2048 + 540 * 2048 == 3317760
    assert extent(64, 1920, 1080, format=NV12, pitch_y=2048, pitch_c=2048) == 64 * 3317760
    # tight NV12: a CbCr row is 2 * cw bytes
    assert extent(2, 7, 9, format=NV12) == 2 * (7 * 9 + 5 * 8)
    # CIF as three planes at 256-byte pitches... 352 does not fit 256: 512 for luma, 256 for the 176-byte chroma rows
    assert extent(1, 352, 288, format=I420, pitch_y=512, pitch_c=256) == 288 * 512 + 2 * 144 * 256
    # a pitch of one plane only
    assert extent(3, 176, 144, format=I420, pitch_y=192) == 3 * (144 * 192 + 2 * 72 * 88)


def test_extent_with_offsets_is_the_end_of_the_last_plane():
    w, h = 176, 144                      # chroma 88 x 72
    # NV12, one grid of 512 bytes: Y of stream s at columns 0 / 256, its CbCr plane below the luma rows
    oy = [0, 256]
    oc = [144 * 512, 144 * 512 + 256]
    assert extent(2, w, h, format=NV12, pitch_y=512, pitch_c=512, offsets_y=oy, offsets_cb=oc) == \
        144 * 512 + 256 + 71 * 512 + 176
    # I420 on two grids: luma at pitch 176, chroma planes at pitch 88 behind all luma
    oy = [0, 176 * 144]
    ocb = [2 * 176 * 144, 2 * 176 * 144 + 2 * 88 * 72]
    ocr = [o + 88 * 72 for o in ocb]
    assert extent(2, w, h, format=I420, offsets_y=oy, offsets_cb=ocb, offsets_cr=ocr) == 2 * (176 * 144 + 2 * 88 * 72)


def test_refusals():
    w, h = 176, 144
    assert refused(1, w, h, format=2)                                            # unknown format
    lay, _ = h263mi.make_yuv_layout(NV12)
    lay.reserved[3] = 1
    assert refused(1, w, h, layout=lay)                                          # reserved byte set
    assert refused(1, w, h, format=I420, pitch_y=175)                            # pitch below the row
    assert refused(1, w, h, format=I420, pitch_c=87)
    assert refused(1, w, h, format=NV12, pitch_c=175)                            # (an NV12 chroma row is 2 * cw bytes)
    assert extent(1, w, h, format=NV12, pitch_c=176) == 176 * 144 + 72 * 176
    # a plane span (rows - 1) * pitch + row at or above 2^32
    big = ((1 << 32) - 176) // 143 + 1
    assert refused(1, w, h, format=I420, pitch_y=big)
    assert (143 * (big - 1) + 176) < (1 << 32) and extent(1, w, h, format=I420, pitch_y=big - 1) > 0
    assert refused(1, w, h, format=NV12, pitch_c=((1 << 32) - 176) // 71 + 1)
    # a row that crosses its pitch boundary: offset % pitch + row > pitch
    assert refused(1, w, h, format=NV12, pitch_y=256, pitch_c=256, offsets_y=[81], offsets_cb=[144 * 256])
    assert extent(1, w, h, format=NV12, pitch_y=256, pitch_c=256, offsets_y=[80], offsets_cb=[144 * 256]) == 144 * 256 + 71 * 256 + 176
    # offsets_cr given for NV12
    assert refused(1, w, h, format=NV12, offsets_y=[0], offsets_cb=[176 * 144], offsets_cr=[176 * 144 + 176 * 72])
    # offset arrays given only in part
    assert refused(1, w, h, format=NV12, offsets_y=[0])
    assert refused(1, w, h, format=NV12, offsets_cb=[176 * 144])
    assert refused(1, w, h, format=I420, offsets_y=[0], offsets_cb=[176 * 144])
    assert refused(1, w, h, format=I420, offsets_cb=[176 * 144], offsets_cr=[176 * 144 + 88 * 72])
    # two planes that share a byte: Cb and Cr of one stream on the chroma grid
    assert refused(1, w, h, format=I420, offsets_y=[0], offsets_cb=[176 * 144], offsets_cr=[176 * 144 + 88 * 71])
    # ... a luma plane's span meeting a chroma plane's across the two grids (the last luma row is the first Cb row and its
    # neighbour; Cb starts on its own grid, so no row crosses a pitch boundary, and Cb and Cr stay apart)
    assert (176 * 144 - 88) % 88 == 0
    assert refused(1, w, h, format=I420, offsets_y=[0], offsets_cb=[176 * 144 - 88], offsets_cr=[176 * 144 - 88 + 88 * 72])
    assert extent(1, w, h, format=I420, offsets_y=[0], offsets_cb=[176 * 144], offsets_cr=[176 * 144 + 88 * 72]) == 176 * 144 + 2 * 88 * 72
    # nothing to lay out
    assert refused(0, w, h, format=I420)
    assert refused(1, 0, h, format=I420)


def _mosaic(n, cols, w, h, pitch, gap_x=0, gap_y=0):
    """NV12 on one grid of `pitch` bytes: tiles of w x (h + ch) -- a picture's CbCr plane right below its luma"""
    ch = (h + 1) // 2
    oy = [(s // cols) * (h + ch + gap_y) * pitch + (s % cols) * (w + gap_x) for s in range(n)]
    oc = [o + h * pitch for o in oy]
    return oy, oc


def test_a_mosaic_that_just_fits_and_one_that_overlaps_by_a_byte_column():
    w, h, n, cols = 176, 144, 4, 2
    pitch = cols * w                                  # no gap: every byte of the grid's rows is some plane's
    oy, oc = _mosaic(n, cols, w, h, pitch)
    rows = 2 * (144 + 72)
    assert extent(n, w, h, format=NV12, pitch_y=pitch, pitch_c=pitch, offsets_y=oy, offsets_cb=oc) == rows * pitch
    # the same with tile 1 moved left by one byte column: its planes now share a column with tile 0's
    oy2, oc2 = list(oy), list(oc)
    oy2[1] -= 1
    oc2[1] -= 1
    assert refused(n, w, h, format=NV12, pitch_y=pitch, pitch_c=pitch, offsets_y=oy2, offsets_cb=oc2)
    # only the chroma plane moved: the luma rectangles are still apart, the CbCr rectangles of tiles 0 and 1 meet
    assert refused(n, w, h, format=NV12, pitch_y=pitch, pitch_c=pitch, offsets_y=oy, offsets_cb=oc2)
    # moved up by one row instead: tile 2's luma lands in tile 0's last CbCr row
    oy3, oc3 = list(oy), list(oc)
    oy3[2] -= pitch
    oc3[2] -= pitch
    assert refused(n, w, h, format=NV12, pitch_y=pitch, pitch_c=pitch, offsets_y=oy3, offsets_cb=oc3)
    # 64 x 1080p as one 8 x 8 NV12 mosaic
    oy, oc = _mosaic(64, 8, 1920, 1080, 8 * 1920)
    assert extent(64, 1920, 1080, format=NV12, pitch_y=8 * 1920, pitch_c=8 * 1920, offsets_y=oy, offsets_cb=oc) == 8 * 1620 * 8 * 1920


def test_the_header_struct_and_the_binding_agree():
    assert C.sizeof(h263mi.YuvLayout) == 48
    assert h263mi.YuvLayout.pitch_y.offset == 8 and h263mi.YuvLayout.offsets_y.offset == 24
    assert h263mi.lib().h263mi_abi_version() == 7
