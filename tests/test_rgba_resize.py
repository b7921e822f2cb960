"""RGBA output resized to any W' x H' (h263mi_rgba_resize): the numpy restatement against hand-derived answers and its
identities, and h263mi_rgba_resize_extent -- a pure host function, so all of this runs without a device."""
import json
import os

import numpy as np
import pytest

import h263mi
import rgba_layout_ref
import rgba_resize_ref as ref

GOLD = os.path.join(os.path.dirname(__file__), "golden", "rgba_resize_known_answers.json")
SIZES = [(1, 1), (5, 4), (7, 9), (176, 144), (352, 288), (1920, 1080)]


def _pic(w, h, seed):
    p = np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)
    p[:, :, 3] = 255
    return p


def test_restatement_matches_known_answers():
    with open(GOLD) as f:
        doc = json.load(f)
    shapes = set()
    for case in doc["cases"]:
        inp = doc["inputs"][case["input"]]
        w, h, ow, oh = inp["w"], inp["h"], case["out_w"], case["out_h"]
        rgba = np.array(inp["rgba"], np.uint8).reshape(h, w, 4)
        assert case["d"] == w * h
        # the weights as written out, and the restatement's
        assert ref.weights(w, ow).tolist() == case["ox"]
        assert ref.weights(h, oh).tolist() == case["oy"]
        got = ref.resize(rgba, w, h, ow, oh)
        assert got.shape == (oh, ow, 4)
        for px in case["pixels"]:
            # the answer file's own arithmetic first, then the restatement
            s = [sum(t[2] * int(rgba[t[0], t[1], c]) for t in px["terms"]) for c in range(3)]
            assert s == px["sum"]
            assert [(v + w * h // 2) // (w * h) for v in s] + [255] == px["out"]
            assert list(got[px["Y"], px["X"]]) == px["out"], (case["input"], px)
        shapes.add((w, h, ow, oh))
    assert {(3, 1, 2, 1), (2, 1, 3, 1), (5, 3, 2, 2)} <= shapes
    assert any(s[2:] == (1, 1) for s in shapes)


@pytest.mark.parametrize("w,h", SIZES)
def test_weights_sum_to_the_source_size(w, h):
    for ow in (1, 3, w, 2 * w + 1):
        wt = ref.weights(w, ow)
        assert (wt.sum(axis=1) == w).all() and (wt.sum(axis=0) == ow).all()


@pytest.mark.parametrize("w,h", SIZES)
def test_identity_at_full_size(w, h):
    p = _pic(w, h, w + h)
    assert (ref.resize(p, w, h, w, h) == p).all()


@pytest.mark.parametrize("w,h", [(4, 4), (8, 12), (176, 144), (352, 288), (1920, 1080)])
def test_equals_box_average_when_f_divides(w, h):
    p = _pic(w, h, 3 * w + h)
    for s in (1, 2):
        f = 1 << s
        if w % f or h % f:
            continue
        assert (ref.resize(p, w, h, w // f, h // f) == rgba_layout_ref.box_average(p, w, h, s)).all()
        assert ref.routed_scale(w, h, w // f, h // f) == s


def test_routing_is_by_sizes_only():
    assert ref.routed_scale(1920, 1080, 1920, 1080) == 0
    assert ref.routed_scale(1920, 1080, 960, 540) == 1
    assert ref.routed_scale(1920, 1080, 480, 270) == 2
    assert ref.routed_scale(1920, 1080, 640, 360) is None
    assert ref.routed_scale(7, 9, 4, 5) is None            # the ceil sizes of 1/2: not the same filter at odd sizes
    assert ref.routed_scale(6, 10, 3, 5) == 1
    assert ref.routed_scale(6, 10, 2, 3) is None


@pytest.mark.parametrize("w,h", SIZES)
def test_constant_stays_constant(w, h):
    for v in (0, 1, 127, 128, 254, 255):
        p = np.full((h, w, 4), v, np.uint8)
        p[:, :, 3] = 255
        for ow, oh in ((1, 1), (3, 2), (w + 3, h + 1), (640, 360)):
            out = ref.resize(p, w, h, ow, oh)
            assert (out[:, :, :3] == v).all() and (out[:, :, 3] == 255).all()


def test_wall_extents():
    # the 3 x 3 wall of 640 x 360 tiles on a 1920 x 1080 canvas
    offs = [(i // 3) * 360 * 7680 + (i % 3) * 640 * 4 for i in range(9)]
    assert h263mi.rgba_resize_extent(9, 640, 360, 7680, offs) == 1920 * 1080 * 4
    # 64 tiles of 640 x 360 in an 8 x 8 canvas of 5120 x 2880
    offs = [(i // 8) * 360 * 20480 + (i % 8) * 2560 for i in range(64)]
    assert h263mi.rgba_resize_extent(64, 640, 360, 20480, offs) == 5120 * 2880 * 4
    for n, ow, oh, pitch in ((1, 1, 1, 0), (3, 7, 5, 0), (64, 640, 360, 0), (2, 320, 180, 4096), (1, 352, 1, 0)):
        want = ref.extent(n, ow, oh, pitch)
        assert want is not None and h263mi.rgba_resize_extent(n, ow, oh, pitch) == want
    assert h263mi.rgba_resize_extent(64, 640, 360) == 64 * 640 * 360 * 4


def _refused(n, ow, oh, reserved=None, **kw):
    r, keep = h263mi.make_rgba_resize(ow, oh, **kw)
    if reserved is not None:
        r.reserved[reserved] = 1
    with pytest.raises(h263mi.H263Error) as e:
        h263mi.rgba_resize_extent(n, ow, oh, resize=r)
    assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    assert ref.extent(n, ow, oh, kw.get("row_pitch", 0), kw.get("offsets"), 1 if reserved is not None else 0) is None
    del keep


def test_each_rule_refuses():
    _refused(1, 0, 16)                                                   # W' = 0
    _refused(1, 16, 0)                                                   # H' = 0
    for k in range(4):
        _refused(1, 16, 16, reserved=k)                                  # a reserved byte set
    _refused(1, 16, 16, row_pitch=60)                                    # below 4W'
    _refused(1, 16, 16, row_pitch=66)                                    # not a multiple of 4
    _refused(2, 16, 16, row_pitch=128, offsets=[0, 66])                  # offset not a multiple of 4
    _refused(2, 16, 16, row_pitch=128, offsets=[0, 72])                  # a row crosses the pitch: 72 + 64 > 128
    _refused(1, 640, 1080, row_pitch=4 * 1024 * 1024)                    # (H'-1) * pitch + 4W' >= 2^32
    _refused(2, 16, 16, row_pitch=128, offsets=[0, 60])                  # overlap in the same rows
    _refused(2, 16, 16, row_pitch=128, offsets=[0, 15 * 128 + 32])       # overlap: last row of 0 / first row of 1
    _refused(0, 16, 16)                                                  # no streams
    with pytest.raises(h263mi.H263Error):                                # no resize at all
        import ctypes as C
        nb = C.c_uint64()
        h263mi._check(h263mi.lib().h263mi_rgba_resize_extent(1, None, C.byref(nb)), "rgba_resize_extent")
    # ... and the neighbours that are fine
    assert h263mi.rgba_resize_extent(2, 16, 16, 128, [0, 64]) == 15 * 128 + 128
    assert h263mi.rgba_resize_extent(2, 16, 16, 128, [0, 16 * 128]) == 31 * 128 + 64
    assert h263mi.rgba_resize_extent(1, 65535, 1) == 4 * 65535
    assert h263mi.rgba_resize_extent(1, 640, 1080, (1 << 32) // 1080 // 4 * 4) is not None
