"""Normalised planar float tensor output (h263mi_tensor_out): the numpy restatement against answers derived in exact rational
arithmetic, and h263mi_tensor_extent -- a pure host function, so all of this runs without a device."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import h263mi
import tensor_out_ref as ref

GOLD = os.path.join(os.path.dirname(__file__), "golden", "tensor_out_known_answers.json")


def _f32(bits):
    return np.array([int(bits, 16)], np.uint32).view(np.float32)[0]


def _cases():
    with open(GOLD) as f:
        return json.load(f)["cases"]


def test_restatement_matches_known_answers():
    names = set()
    fused_differs = 0
    for c in _cases():
        dtype = ref.NAMES[c["dtype"]]
        scale, bias = _f32(c["scale_bits"]), _f32(c["bias_bits"])
        with np.errstate(over="ignore"):
            v = ref.values(np.array([c["u"]], np.uint8), scale, bias)
        got = int(ref.bits(v, dtype)[0])
        assert got == int(c["bits"], 16), (c["name"], hex(got), c["bits"])
        names.add(c["name"])
        if c["name"].startswith("fused_would_differ"):
            # the case is what it says: one rounding gives another binary32 than the definition's two
            assert c["dtype"] == "f32" and c["fused_f32_bits"] != c["bits"]
            fused_differs += 1
    assert {"f16_tie_down_to_even", "f16_tie_up_to_even", "bf16_tie_down_to_even", "bf16_tie_up_to_even", "f16_subnormal",
            "bf16_subnormal", "f32_subnormal", "f16_overflow"} <= names
    assert fused_differs >= 1


def test_planes_follow_colour_order_and_per_colour_parameters():
    rgba = np.zeros((2, 3, 4), np.uint8)
    rgba[:, :, 0], rgba[:, :, 1], rgba[:, :, 2], rgba[:, :, 3] = 10, 20, 30, 255
    scale, bias = (1.0, 2.0, 3.0), (0.5, 0.25, 0.125)
    rgb = ref.planes(rgba, ref.F32, scale, bias).view(np.float32)
    assert rgb.shape == (3, 2, 3)
    assert [float(rgb[p, 0, 0]) for p in range(3)] == [10.5, 40.25, 90.125]
    bgr = ref.planes(rgba, ref.F32, scale, bias, bgr=True).view(np.float32)
    assert [float(bgr[p, 1, 2]) for p in range(3)] == [90.125, 40.25, 10.5]        # scale and bias stay with their colour
    canvas = np.full(64, 0xAAAA, np.uint16)
    ref.place(canvas, ref.planes(rgba, ref.BF16, scale, bias), base=1, stride_c=11, stride_h=4)
    touched = np.nonzero(canvas != 0xAAAA)[0].tolist()
    assert touched == [1 + p * 11 + y * 4 + x for p in range(3) for y in range(2) for x in range(3)]


def _extent(n, t):
    nb = C.c_uint64(0xDEAD)
    rc = h263mi.lib().h263mi_tensor_extent(n, C.byref(t) if t is not None else None, C.byref(nb))
    return nb.value if rc == h263mi.OK else (None if rc == h263mi.ERR_INVALID_ARGUMENT else rc)


def _t(ow=5, oh=3, dtype=ref.F32, **kw):
    return h263mi.make_tensor_out(ow, oh, dtype, **kw)


@pytest.mark.parametrize("dtype", [ref.F32, ref.F16, ref.BF16])
def test_extent_default_and_given_strides(dtype):
    e = ref.ELT[dtype]
    assert _extent(1, _t(dtype=dtype)) == e * 3 * 3 * 5
    assert _extent(4, _t(dtype=dtype)) == e * 4 * 3 * 3 * 5
    assert _extent(4, _t(224, 224, dtype)) == e * 4 * 3 * 224 * 224
    # padded: elt * ((n-1)*stride_n + 2*stride_c + (H'-1)*stride_h + W')
    t = _t(dtype=dtype, stride_h=8, stride_c=29, stride_n=94)
    assert _extent(3, t) == e * (2 * 94 + 2 * 29 + 2 * 8 + 5) == ref.extent(3, 5, 3, dtype, stride_n=94, stride_c=29, stride_h=8)
    # the defaults build on the strides that are given: stride_c = H' * stride_h, stride_n = 3 * stride_c
    assert _extent(2, _t(dtype=dtype, stride_h=8)) == e * (3 * 24 + 2 * 24 + 2 * 8 + 5)
    assert _extent(2, _t(dtype=dtype, stride_c=40)) == e * (120 + 80 + 2 * 5 + 5)
    # the tightest strides that pass
    assert _extent(2, _t(dtype=dtype, stride_h=5, stride_c=15, stride_n=45)) == e * 90
    # stride_n is not looked at for one stream
    assert _extent(1, _t(dtype=dtype, stride_n=1)) == e * 45


def test_extent_refusals():
    assert _extent(1, None) is None
    assert _extent(0, _t()) is None
    assert _extent(1, _t(ow=0)) is None
    assert _extent(1, _t(oh=0)) is None
    assert _extent(1, _t(dtype=3)) is None
    assert _extent(1, _t(dtype=255)) is None
    t = _t()
    t.bgr = 2
    assert _extent(1, t) is None
    for k in range(2):
        t = _t()
        t.reserved[k] = 1
        assert _extent(1, t) is None
    for bad in (float("inf"), float("-inf"), float("nan")):
        for k in range(3):
            s, b = [1.0, 1.0, 1.0], [0.0, 0.0, 0.0]
            s[k] = bad
            assert _extent(1, _t(scale=s)) is None
            b[k] = bad
            assert _extent(1, _t(bias=b)) is None
    assert _extent(1, _t(stride_h=4)) is None                         # stride_h < W'
    assert _extent(1, _t(stride_h=5)) == 4 * 45
    assert _extent(1, _t(stride_c=14)) is None                        # stride_c < (H'-1)*stride_h + W' = 15
    assert _extent(1, _t(stride_h=8, stride_c=20)) is None            # ... = 21
    assert _extent(1, _t(stride_h=8, stride_c=21)) == 4 * (42 + 21)
    assert _extent(2, _t(stride_n=44)) is None                        # stride_n < 2*stride_c + (H'-1)*stride_h + W' = 45
    assert _extent(2, _t(stride_n=45)) == 4 * 90
    assert _extent(1, _t(stride_n=44)) == 4 * 45                      # ... only while n_streams > 1
    # subnormal scale and bias are finite
    assert _extent(1, _t(scale=(1e-45, 1, 1), bias=(-1e-45, 0, 0))) == 4 * 45


def test_extent_one_picture_below_4_gib():
    # one picture's byte span must stay below 2^32: 2*stride_c + (H'-1)*stride_h + W' elements
    for dtype, e in ((ref.F32, 4), (ref.F16, 2)):
        lim = (1 << 32) // e                                            # elements: the span must be < lim
        sc = (lim - 15) // 2
        assert 2 * sc + 15 == lim - 1
        assert _extent(1, _t(dtype=dtype, stride_c=sc)) == e * (lim - 1) == ref.extent(1, 5, 3, dtype, stride_c=sc)
        assert _extent(1, _t(dtype=dtype, stride_c=sc + 1)) is None and ref.extent(1, 5, 3, dtype, stride_c=sc + 1) is None
    # the largest sizes with default strides: 3 * 65535^2 elements is far beyond
    assert _extent(1, _t(65535, 65535)) is None
    assert _extent(1, _t(65535, 5461)) == 4 * 3 * 65535 * 5461
    assert _extent(1, _t(65535, 5462)) is None


def test_extent_arithmetic_does_not_wrap():
    big = 1 << 63
    # strides near 2^63 and 2^64: every product and sum would wrap 64 bits; all are refused, none comes back small
    for kw in (dict(stride_h=big), dict(stride_c=big), dict(stride_h=(1 << 64) - 1), dict(stride_c=(1 << 64) - 1),
               dict(stride_h=big, stride_c=big), dict(stride_h=big + 1, stride_c=(1 << 64) - 1)):
        assert _extent(1, _t(**kw)) is None, kw
        assert ref.extent(1, 5, 3, **kw) is None
    # stride_n alone may be huge while the total fits 64 bits
    sn = (1 << 61)
    assert _extent(2, _t(stride_n=sn)) == 4 * (sn + 45) == ref.extent(2, 5, 3, stride_n=sn)
    assert _extent(3, _t(dtype=ref.F16, stride_n=sn)) == 2 * (2 * sn + 45)
    # ... and is refused once (n-1) * stride_n * elt passes 2^64, however it wraps
    assert _extent(3, _t(stride_n=sn)) is None and ref.extent(3, 5, 3, stride_n=sn) is None      # 2 * 2^61 * 4 = 2^64 exactly
    assert _extent(5, _t(stride_n=sn)) is None and ref.extent(5, 5, 3, stride_n=sn) is None      # 2^65: wraps to 180
    assert _extent(3, _t(stride_n=big)) is None                                                # 2 * 2^63 * 4: wraps to 180
    assert _extent(2, _t(stride_n=(1 << 64) - 1)) is None
    assert _extent(0xFFFFFFFF, _t(stride_n=(1 << 64) - 1)) is None
    assert _extent(0xFFFFFFFF, _t(dtype=ref.BF16)) == 2 * 0xFFFFFFFF * 45
    # the last total that fits, and the first that does not (2-byte elements)
    sn = ((1 << 63) - 45)                                               # 2 * (sn + 45) = 2^64
    assert _extent(2, _t(dtype=ref.F16, stride_n=sn)) is None
    assert _extent(2, _t(dtype=ref.F16, stride_n=sn - 1)) == (1 << 64) - 2


def test_python_wrapper_raises_on_refusal():
    assert h263mi.tensor_extent(2, _t()) == 4 * 90
    with pytest.raises(h263mi.H263Error) as e:
        h263mi.tensor_extent(1, _t(stride_h=1))
    assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
