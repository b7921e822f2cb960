"""numpy restatement of the normalised planar float tensor output (include/h263mi.h: h263mi_tensor_out) -- TEST INFRASTRUCTURE.

values(u, scale, bias): fl32(fl32(float32(u) * scale) + bias) -- two numpy.float32 operations, each rounded to nearest even,
    subnormals kept -- as a float32 array.
bits(v, dtype): the element's bit pattern: float32 as uint32; "f16": v.astype(float16) as uint16 (round to nearest even,
    overflow to +-inf, subnormals kept); "bf16": (b + 0x7fff + ((b >> 16) & 1)) >> 16 of the float32 bits b, as uint16.
planes(rgba, dtype, scale, bias, bgr): the W' x H' RGBA of rgba_resize_ref.resize -> (3, H', W') bit patterns; plane p holds
    colour p, or 2 - p with bgr; scale and bias are per COLOUR.
place(canvas, planes, base, stride_c, stride_h): the planes written into a 1-D canvas of elements at element `base`.
extent(...): h263mi_tensor_extent restated (None where it answers H263MI_ERR_INVALID_ARGUMENT).
Pinned by tests/golden/tensor_out_known_answers.json (tests/test_tensor_out.py).
"""
import math

import numpy as np

F32, F16, BF16 = 0, 1, 2
NAMES = {"f32": F32, "f16": F16, "bf16": BF16}
ELT = {F32: 4, F16: 2, BF16: 2}
BITS_DTYPE = {F32: np.uint32, F16: np.uint16, BF16: np.uint16}
# (scale, bias) per colour: ImageNet's normalisation, 1 / (255 * std) and -mean / std; and a set that reaches binary16 and
# bfloat16 subnormals (red, blue), binary16 overflow (green) and binary32 subnormals (blue)
IMAGENET = ([1 / (255 * 0.229), 1 / (255 * 0.224), 1 / (255 * 0.225)], [-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225])
EDGES = ([2.0 ** -24 * 0.37, 400.0, 2.0 ** -133 * 1.7], [2.0 ** -20, -32000.0, -2.0 ** -131])


def values(u, scale, bias):
    u = np.asarray(u).astype(np.float32)
    m = (u * np.float32(scale)).astype(np.float32)
    return (m + np.float32(bias)).astype(np.float32)


def bits(v, dtype):
    v = np.ascontiguousarray(v, np.float32)
    b = v.view(np.uint32)
    if dtype == F32:
        return b.copy()
    if dtype == F16:
        with np.errstate(over="ignore"):
            return v.astype(np.float16).view(np.uint16)
    b = b.astype(np.uint64)
    return ((b + 0x7fff + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def planes(rgba, dtype, scale, bias, bgr=False):
    """rgba: (H', W', 4) uint8 -> (3, H', W') bit patterns"""
    rgba = np.asarray(rgba, np.uint8)
    with np.errstate(over="ignore"):
        out = [bits(values(rgba[:, :, c], scale[c], bias[c]), dtype) for c in range(3)]
    if bgr:
        out = out[::-1]
    return np.stack(out)


def place(canvas, pl, base=0, stride_c=0, stride_h=0):
    """writes the (3, H', W') planes into the 1-D element canvas; returns it"""
    _, H, W = pl.shape
    sh = stride_h or W
    sc = stride_c or H * sh
    for p in range(3):
        for y in range(H):
            at = base + p * sc + y * sh
            canvas[at:at + W] = pl[p, y]
    return canvas


def extent(n, ow, oh, dtype=F32, bgr=0, reserved=(0, 0), scale=(1, 1, 1), bias=(0, 0, 0), stride_n=0, stride_c=0, stride_h=0):
    """bytes of h263mi_tensor_extent, or None where it answers H263MI_ERR_INVALID_ARGUMENT (Python integers: nothing wraps)"""
    if n == 0 or ow == 0 or oh == 0 or dtype not in ELT or bgr > 1 or any(reserved):
        return None
    if not all(math.isfinite(float(np.float32(v))) for v in tuple(scale) + tuple(bias)):
        return None
    sh = stride_h or ow
    if sh < ow:
        return None
    plane = (oh - 1) * sh + ow
    sc = stride_c or oh * sh
    if sc < plane:
        return None
    picture = 2 * sc + plane
    if picture * ELT[dtype] >= 1 << 32:
        return None
    sn = stride_n or 3 * sc
    if n > 1 and sn < picture:
        return None
    total = ELT[dtype] * ((n - 1) * sn + picture)
    return total if total < 1 << 64 else None
