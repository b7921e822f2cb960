"""RGBA output layout (h263mi_rgba_layout): the numpy restatement against hand-derived answers, and
h263mi_rgba_layout_extent -- a pure host function, so all of this runs without a device."""
import json
import os

import numpy as np
import pytest

import h263mi
import rgba_layout_ref as ref

GOLD = os.path.join(os.path.dirname(__file__), "golden", "rgba_layout_known_answers.json")
SIZES = [(1, 1), (5, 4), (7, 9), (176, 144), (352, 288), (1920, 1080)]


def _gold():
    with open(GOLD) as f:
        return json.load(f)


def test_restatement_matches_known_answers():
    doc = _gold()
    seen_n = set()
    ties = 0
    for case in doc["cases"]:
        inp = doc["inputs"][case["input"]]
        w, h = inp["w"], inp["h"]
        rgba = np.array(inp["rgba"], np.uint8)
        got = ref.box_average(rgba, w, h, case["scale_log2"])
        assert got.shape == (case["out_h"], case["out_w"], 4)
        for b in case["boxes"]:
            # the answer file's own arithmetic first, then the restatement
            assert [(s + b["n"] // 2) // b["n"] for s in b["sum"]] + [255] == b["out"]
            assert list(got[b["Y"], b["X"]]) == b["out"], (case["input"], case["scale_log2"], b)
            seen_n.add(b["n"])
            ties += bool(b.get("tie"))
    assert {1, 2, 3, 6, 9, 12} <= seen_n
    assert ties > 0


def test_restatement_scale_1_is_identity():
    rgba = np.random.default_rng(1).integers(0, 256, (9, 7, 4), dtype=np.uint8)
    rgba[:, :, 3] = 255
    assert (ref.box_average(rgba, 7, 9, 0) == rgba).all()


def _pitches(w, s):
    ow, _ = ref.out_size(w, 1, s)
    return [0, 4 * ow, 4 * ow + 4, ((4 * ow + 255) // 256) * 256, 8192]


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("s", [0, 1, 2])
def test_extent_table(w, h, s):
    for pitch in _pitches(w, s):
        for n in (1, 3, 64):
            want = ref.extent(n, w, h, s, pitch)
            assert want is not None
            assert h263mi.rgba_layout_extent(n, w, h, s, pitch) == want
    ow, oh = ref.out_size(w, h, s)
    assert h263mi.rgba_layout_extent(1, w, h, s, 0)[:2] == (ow, oh)


@pytest.mark.parametrize("w,h", SIZES)
def test_default_layout_extent_is_today(w, h):
    for n in (1, 2, 64):
        assert h263mi.rgba_layout_extent(n, w, h) == (w, h, n * w * h * 4)
        ow, oh, nb = C_extent_null(n, w, h)
        assert (ow, oh, nb) == (w, h, n * w * h * 4)


def C_extent_null(n, w, h):
    """h263mi_rgba_layout_extent with a NULL layout"""
    import ctypes as C
    ow, oh, nb = C.c_uint16(), C.c_uint16(), C.c_uint64()
    rc = h263mi.lib().h263mi_rgba_layout_extent(n, w, h, None, C.byref(ow), C.byref(oh), C.byref(nb))
    assert rc == h263mi.OK
    return ow.value, oh.value, nb.value


def test_mosaic_extents():
    offs = [(i // 8) * 270 * 15360 + (i % 8) * 480 * 4 for i in range(64)]
    assert h263mi.rgba_layout_extent(64, 1920, 1080, 2, 15360, offs) == (480, 270, 3840 * 2160 * 4)
    offs = [(i // 4) * 144 * 2816 + (i % 4) * 704 for i in range(16)]      # CIF at 1/2: 4 x 4 tiles of 176 x 144
    assert h263mi.rgba_layout_extent(16, 352, 288, 1, 2816, offs) == (176, 144, 576 * 2816)
    assert ref.extent(64, 1920, 1080, 2, 15360, [(i // 8) * 270 * 15360 + (i % 8) * 1920 for i in range(64)])[2] == 3840 * 2160 * 4


def _refused(n, w, h, **kw):
    reserved = kw.pop("reserved", None)
    lay, keep = h263mi.make_rgba_layout(**kw)
    if reserved is not None:
        lay.reserved[reserved] = 1
    with pytest.raises(h263mi.H263Error) as e:
        h263mi.rgba_layout_extent(n, w, h, layout=lay)
    assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    assert ref.extent(n, w, h, kw.get("scale_log2", 0), kw.get("row_pitch", 0), kw.get("offsets"),
                      1 if reserved is not None else 0) is None
    del keep


def test_each_rule_refuses():
    _refused(1, 16, 16, scale_log2=3)                                   # scale beyond 1/4
    for k in range(7):
        _refused(1, 16, 16, reserved=k)                                 # a reserved byte set
    _refused(1, 16, 16, row_pitch=60)                                   # below 4W'
    _refused(1, 16, 16, row_pitch=66)                                   # not a multiple of 4
    _refused(2, 16, 16, row_pitch=128, offsets=[0, 66])                 # offset not a multiple of 4
    _refused(2, 16, 16, row_pitch=128, offsets=[0, 72])                 # a row crosses the pitch: 72 + 64 > 128
    _refused(1, 1920, 1080, row_pitch=4 * 1024 * 1024)                  # (H'-1) * pitch + 4W' >= 2^32
    _refused(2, 16, 16, row_pitch=128, offsets=[0, 60])                 # overlap in the same rows
    _refused(2, 16, 16, row_pitch=128, offsets=[0, 15 * 128 + 32])      # overlap: last row of 0 / first row of 1
    _refused(2, 16, 16, scale_log2=1, row_pitch=64, offsets=[0, 7 * 64 + 28])   # 1/2 scale: 8 rows of 32 bytes
    _refused(0, 16, 16)
    # ... and the neighbours that are fine
    assert h263mi.rgba_layout_extent(2, 16, 16, 0, 128, [0, 64]) == (16, 16, 15 * 128 + 128)
    assert h263mi.rgba_layout_extent(2, 16, 16, 0, 128, [0, 16 * 128]) == (16, 16, 31 * 128 + 64)
    assert h263mi.rgba_layout_extent(2, 16, 16, 1, 64, [0, 8 * 64]) == (8, 8, 15 * 64 + 32)
    assert h263mi.rgba_layout_extent(1, 1920, 1080, 0, (1 << 32) // 1080 // 4 * 4) is not None


def test_placement_restatement_keeps_the_gaps():
    pics = [np.full((3, 2, 4), 10 + i, np.uint8) for i in range(4)]
    offs = [0, 12, 3 * 32, 3 * 32 + 12]
    canvas = ref.place(np.full(6 * 32, 0xEE, np.uint8), pics, 32, offs)
    m = ref.rect_mask(canvas.size, 2, 3, 0, 32, offs)
    assert (canvas[~m] == 0xEE).all() and m.sum() == 4 * 3 * 8
    assert (canvas[:8] == 10).all() and (canvas[12:20] == 11).all() and (canvas[96:104] == 12).all()
