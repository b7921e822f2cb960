"""Deblocked planes resized to any W' x H' (h263mi_yuv_resize): the numpy restatement against hand-derived answers and its
identities, and h263mi_yuv_resize_extent -- a pure host function, so all of this runs without a device."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import h263mi
import yuv_layout_ref as lay
import yuv_resize_ref as ref

GOLD = os.path.join(os.path.dirname(__file__), "golden", "yuv_resize_known_answers.json")
FORMATS = [h263mi.YUV_I420, h263mi.YUV_NV12]


def _doc():
    with open(GOLD) as f:
        return json.load(f)


def test_restatement_matches_known_answers():
    doc = _doc()
    shapes = set()
    for case in doc["planes"]:
        pw, ph, ow, oh = case["pw"], case["ph"], case["ow"], case["oh"]
        names = dict(zip("abcd", case["plane"]))
        # the answer file's own formulas first, then the restatement
        assert [eval(f, {"__builtins__": {}}, names) for f in case["formula"]] == case["out"], case["name"]
        got = ref.resize_plane(np.array(case["plane"], np.uint8), pw, ph, ow, oh)
        assert got.shape == (oh, ow) and got.ravel().tolist() == case["out"], case["name"]
        assert case["why"]
        shapes.add((pw, ph, ow, oh))
    assert shapes == {(3, 1, 2, 1), (2, 2, 1, 1), (1, 1, 3, 2)}


@pytest.mark.parametrize("pw,ph", [(1, 1), (5, 4), (7, 9), (176, 144)])
def test_constant_planes_stay_constant(pw, ph):
    for v in _doc()["constants"]["values"] + [1, 127, 128, 254]:
        p = np.full(pw * ph, v, np.uint8)
        for ow, oh in ((1, 1), (3, 2), (pw + 3, ph + 1), (100, 37)):
            assert (ref.resize_plane(p, pw, ph, ow, oh) == v).all()


def test_bookkeeping_of_odd_sizes():
    bk = _doc()["bookkeeping"]
    ow, oh = bk["out_width"], bk["out_height"]
    assert lay.chroma_size(ow, oh) == (bk["chroma_width"], bk["chroma_height"])
    assert lay.row_bytes(ow, lay.NV12)[1] == bk["nv12_chroma_row_bytes"]
    assert lay.row_bytes(ow, lay.I420)[1] == bk["i420_chroma_row_bytes"]
    assert h263mi.yuv_resize_extent(1, ow, oh, h263mi.YUV_NV12) == bk["nv12_bytes"] == ref.extent(1, ow, oh, ref.NV12)
    assert h263mi.yuv_resize_extent(1, ow, oh, h263mi.YUV_I420) == bk["i420_bytes"] == ref.extent(1, ow, oh, ref.I420)
    # all three planes of a 7 x 9 picture to 5 x 3: the chroma planes are resized from 4 x 5 to 3 x 2
    rng = np.random.default_rng(1)
    planes = (rng.integers(0, 256, 63, dtype=np.uint8), rng.integers(0, 256, 20, dtype=np.uint8), rng.integers(0, 256, 20, dtype=np.uint8))
    y, cb, cr = ref.resize_planes(planes, 7, 9, ow, oh)
    assert (y.size, cb.size, cr.size) == (15, 6, 6)
    assert (cb == ref.resize_plane(planes[1], 4, 5, 3, 2).ravel()).all()


@pytest.mark.parametrize("w,h", [(1, 1), (5, 4), (7, 9), (176, 144)])
def test_identity_at_full_size(w, h):
    cw, ch = lay.chroma_size(w, h)
    rng = np.random.default_rng(w + h)
    planes = tuple(rng.integers(0, 256, k, dtype=np.uint8) for k in (w * h, cw * ch, cw * ch))
    for got, want in zip(ref.resize_planes(planes, w, h, w, h), planes):
        assert (got == want).all()


def _lib_extent(n, ow, oh, fmt, py, pc, oy, ocb, ocr, reserved=None):
    r, keep = h263mi.make_yuv_resize(ow, oh, fmt, py, pc, oy, ocb, ocr)
    if reserved is not None:
        r.reserved[reserved] = 1
    nb = C.c_uint64()
    rc = h263mi.lib().h263mi_yuv_resize_extent(n, C.byref(r), C.byref(nb))
    del keep
    assert rc in (h263mi.OK, h263mi.ERR_INVALID_ARGUMENT)
    return nb.value if rc == h263mi.OK else None


def test_extent_against_the_restatement_over_a_seeded_sweep():
    rng = np.random.default_rng(20240)
    accepted = refused = 0
    for _ in range(1500):
        n = int(rng.integers(1, 5))
        ow, oh = int(rng.integers(1, 40)), int(rng.integers(1, 30))
        fmt = int(rng.integers(0, 2))
        ry, rc = lay.row_bytes(ow, fmt)
        ch = (oh + 1) // 2
        # pitches: tight, exact, padded, sometimes one byte short of the row; sometimes one pitch for both planes
        py = int(rng.choice([0, ry, ry + int(rng.integers(0, 3 * ry + 9)), max(1, ry - 1)], p=[0.3, 0.2, 0.4, 0.1]))
        pc = int(rng.choice([0, rc, rc + int(rng.integers(0, 3 * rc + 9)), max(1, rc - 1)], p=[0.3, 0.2, 0.4, 0.1]))
        if rng.random() < 0.3:
            pc = py = max(py or ry, pc or rc) + int(rng.integers(0, 40))
        kind = rng.random()
        oy = ocb = ocr = None
        if kind < 0.6:
            # offsets that mostly tile (the default placement, shuffled and nudged), sometimes colliding or crossing a pitch
            doy, docb, docr = lay.default_offsets(n, ow, oh, fmt, py, pc)
            perm = rng.permutation(n)
            oy, ocb = [doy[i] for i in perm], [docb[i] for i in perm]
            ocr = None if docr is None else [docr[i] for i in perm]
            if rng.random() < 0.5:
                which = [oy, ocb] + ([ocr] if ocr is not None else [])
                which[int(rng.integers(0, len(which)))][int(rng.integers(0, n))] += int(rng.integers(-ry, 2 * ry + 1))
                for a in which:
                    for i in range(n):
                        a[i] = max(0, a[i])
            if rng.random() < 0.1:
                ocb = None                                            # offset arrays in part
            elif fmt == lay.NV12 and rng.random() < 0.15:
                ocr = list(ocb)                                       # NV12 with offsets_cr
        want = ref.extent(n, ow, oh, fmt, py, pc, oy, ocb, ocr)
        got = _lib_extent(n, ow, oh, fmt, py, pc, oy, ocb, ocr)
        assert got == want, (n, ow, oh, fmt, py, pc, oy, ocb, ocr)
        accepted += want is not None
        refused += want is None
    assert accepted > 300 and refused > 300


def _refused(n, ow, oh, fmt=h263mi.YUV_I420, py=0, pc=0, oy=None, ocb=None, ocr=None, reserved=None):
    assert _lib_extent(n, ow, oh, fmt, py, pc, oy, ocb, ocr, reserved) is None
    assert ref.extent(n, ow, oh, fmt, py, pc, oy, ocb, ocr, 1 if reserved is not None else 0) is None


def test_each_rule_refuses():
    nb = C.c_uint64()
    assert h263mi.lib().h263mi_yuv_resize_extent(1, None, C.byref(nb)) == h263mi.ERR_INVALID_ARGUMENT      # r == NULL
    _refused(0, 16, 16)                                                  # no streams
    _refused(1, 0, 16)                                                   # W' = 0
    _refused(1, 16, 0)                                                   # H' = 0
    for k in range(3):
        _refused(1, 16, 16, reserved=k)                                  # a reserved byte set
    _refused(1, 16, 16, fmt=2)                                           # an unknown format
    # ... and every refusal of h263mi_yuv_layout_extent, for the W' x H' picture
    _refused(1, 16, 16, py=15)                                           # a pitch below its row: luma
    _refused(1, 16, 16, pc=7)                                            # ... chroma, I420 (cW' = 8)
    _refused(1, 16, 16, fmt=h263mi.YUV_NV12, pc=15)                      # ... chroma, NV12 (2 cW' = 16)
    _refused(1, 17, 16, fmt=h263mi.YUV_NV12, pc=17)                      # ... W' = 17: cW' = 9, an NV12 row is 18 bytes
    _refused(1, 16, 16, py=32, pc=8, oy=[20], ocb=[1024], ocr=[2048])    # a row crossing its pitch: 20 + 16 > 32
    _refused(1, 16, 16, py=16, pc=32, oy=[0], ocb=[256 + 28], ocr=[1024])  # ... a chroma row: 28 + 8 > 32
    _refused(1, 16, 16, fmt=h263mi.YUV_NV12, oy=[0], ocb=[256], ocr=[512])  # NV12 with offsets_cr
    _refused(1, 16, 16, oy=[0])                                          # offset arrays in part
    _refused(1, 16, 16, oy=[0], ocb=[256])                               # ... I420 needs all three
    _refused(1, 16, 16, fmt=h263mi.YUV_NV12, ocb=[256])                  # ... NV12 needs both
    _refused(2, 16, 16, oy=[0, 128], ocb=[4096, 4160], ocr=[8192, 8256])  # two luma planes sharing rows 8..15
    _refused(1, 16, 16, py=16, pc=8, oy=[0], ocb=[252], ocr=[1024])      # luma / chroma span overlap under different pitches
    _refused(1, 16, 16, py=16, pc=16, oy=[0], ocb=[15 * 16 + 8], ocr=[1024])  # one grid: Cb on luma's last row, columns 8..15
    _refused(1, 640, 1080, py=4 * 1024 * 1024)                           # a plane span of 2^32 bytes or more
    # ... and the neighbours that are fine
    assert _lib_extent(1, 16, 16, 0, 16, 8, [0], [256], [1024], None) == 1024 + 64
    assert _lib_extent(1, 16, 16, 0, 32, 32, [0], [16], [16 + 8 * 32], None) == 16 + 8 * 32 + 7 * 32 + 8   # one grid, side by side
    assert _lib_extent(1, 65535, 1, 1, 0, 0, None, None, None, None) == 65535 + 65536
    assert h263mi.yuv_resize_extent(64, 640, 360, h263mi.YUV_NV12) == 64 * 640 * 360 * 3 // 2


@pytest.mark.parametrize("w,h", [(1, 1), (5, 4), (7, 9), (176, 144), (1920, 1080)])
def test_full_size_extent_is_the_layout_extent(w, h):
    seen = set()
    for fmt in FORMATS:
        ry, rc = lay.row_bytes(w, fmt)
        for py, pc in ((0, 0), (ry + 5, rc + 3), (2 * ry + 64, 2 * ry + 64)):
            for n in (1, 3):
                assert h263mi.yuv_resize_extent(n, w, h, fmt, py, pc) == h263mi.yuv_layout_extent(n, w, h, fmt, py, pc)
                offs = lay.default_offsets(n, w, h, fmt, py, pc)
                offs = [None if o is None else [v + 7 * (py or ry) * (pc or rc) for v in o] for o in offs]
                # (explicit offsets are held to the pitch grid, which the default placement is not: both refuse alike)
                try:
                    want = h263mi.yuv_layout_extent(n, w, h, fmt, py, pc, *offs)
                except h263mi.H263Error:
                    want = None
                assert _lib_extent(n, w, h, fmt, py, pc, *offs) == want
                seen.add(want is not None)
    assert True in seen


def test_a_ladder_of_nv12_rungs_in_one_buffer():
    """64 streams as 640 x 360 NV12 tiles of an 8 x 8 wall: a 5120-byte pitch, each tile's CbCr plane below its luma plane"""
    pitch = 8 * 640
    oy = [(s // 8) * 540 * pitch + (s % 8) * 640 for s in range(64)]
    oc = [o + 360 * pitch for o in oy]
    assert h263mi.yuv_resize_extent(64, 640, 360, h263mi.YUV_NV12, pitch, pitch, oy, oc) == 8 * 540 * pitch
    assert ref.extent(64, 640, 360, ref.NV12, pitch, pitch, oy, oc) == 8 * 540 * pitch
