"""Restatement of the bilinear and bicubic resampling of a resized output (include/h263mi.h: h263mi_filter) in Python floats
(IEEE binary64, no fused multiply-add) and numpy integers -- TEST INFRASTRUCTURE.

taps(kind, n_in, n_out): h263mi_filter_taps -> (ksize, first[n_out], count[n_out], coeffs[n_out, ksize]) in units of 2^-22, or
    None where it answers H263MI_ERR_INVALID_ARGUMENT.
axis_pass(img, axis, tp, stats): one pass, out = clamp((2^21 + sum coeff * P) >> 22, 0, 255) per channel; stats (a dict, may be
    None) counts the values that were clamped at 0 ("lo") and at 255 ("hi").
resize(img, ow, oh, kind): (h, w, C) uint8 -> (oh, ow, C): the horizontal pass, 8-bit values, then the vertical pass; a pass
    whose two sizes agree is skipped.  It is PIL.Image.resize for mode RGB (tests/test_filter.py holds it to that).
resize_single_rounding(img, ow, oh, kind): the same taps applied as ONE weighted sum with one rounding -- what the contract is
    not; the cases must hold pixels where the two differ (filter_cases.content_hazards).
rgba(full, ow, oh, rects, kind, pad, canvas): the W' x H' RGBA of a framing: resize of the source window (its own edges clamp
    the taps: crop, then resize), pasted at (dx, dy) into a canvas of the pad colour (alpha 255) -- or into `canvas`.
tensor(...): tensor_out_ref.planes of rgba(...).
"""
import math

import numpy as np

import tensor_out_ref

AREA, BILINEAR, BICUBIC = 0, 1, 2
KINDS = {"bilinear": BILINEAR, "bicubic": BICUBIC}
PRECISION = 22
SUPPORT = {BILINEAR: 1.0, BICUBIC: 2.0}


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


_FILTER = {BILINEAR: _bilinear, BICUBIC: _bicubic}
_taps = {}


def taps(kind, n_in, n_out):
    if kind not in _FILTER or not 1 <= n_in <= 65535 or not 1 <= n_out <= 65535:
        return None
    key = (kind, n_in, n_out)
    if key in _taps:
        return _taps[key]
    f = _FILTER[kind]
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = SUPPORT[kind] * fs
    ksize = 2 * int(math.ceil(support)) + 1
    ss = 1.0 / fs
    first = np.zeros(n_out, np.int64)
    count = np.zeros(n_out, np.int64)
    coeffs = np.zeros((n_out, ksize), np.int64)
    for X in range(n_out):
        center = (X + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(n_in, int(center + support + 0.5))
        n = xmax - xmin
        k = [f((i + xmin - center + 0.5) * ss) for i in range(n)]
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        first[X], count[X] = xmin, n
        coeffs[X, :n] = [int(v * 4194304 + 0.5) if v >= 0 else int(v * 4194304 - 0.5) for v in k]
    _taps[key] = (ksize, first, count, coeffs)
    return _taps[key]


def _sums(img, axis, tp):
    """the unrounded weighted sums of one pass, int64, in units of 2^-22"""
    _, first, count, coeffs = tp
    src = np.moveaxis(np.asarray(img).astype(np.int64), axis, 0)
    out = np.zeros((len(first),) + src.shape[1:], np.int64)
    for X in range(len(first)):
        n = int(count[X])
        out[X] = np.tensordot(coeffs[X, :n], src[first[X]:first[X] + n], axes=(0, 0))
    return np.moveaxis(out, 0, axis)


def axis_pass(img, axis, tp, stats=None, mask=False):
    v = (_sums(img, axis, tp) + (1 << (PRECISION - 1))) >> PRECISION
    if stats is not None:
        stats["lo"] = stats.get("lo", 0) + int((v < 0).sum())
        stats["hi"] = stats.get("hi", 0) + int((v > 255).sum())
    return (v & 0xff).astype(np.uint8) if mask else np.clip(v, 0, 255).astype(np.uint8)


def resize(img, ow, oh, kind, stats=None, mutant=None):
    """stats (may be None): {"h": {...}, "v": {...}} of axis_pass.  mutant: None; "single": resize_single_rounding; "mask": the
    horizontal pass keeps the low 8 bits of a value outside 0..255 instead of clamping it"""
    if mutant == "single":
        return resize_single_rounding(img, ow, oh, kind)
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    st = stats if stats is not None else {}
    if ow != w:
        img = axis_pass(img, 1, taps(kind, w, ow), st.setdefault("h", {}), mask=mutant == "mask")
    if oh != h:
        img = axis_pass(img, 0, taps(kind, h, oh), st.setdefault("v", {}))
    return img


def resize_single_rounding(img, ow, oh, kind):
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    v, shift = img.astype(np.int64), 0
    if ow != w:
        v, shift = _sums(v, 1, taps(kind, w, ow)), shift + PRECISION
    if oh != h:
        v, shift = _sums(v, 0, taps(kind, h, oh)), shift + PRECISION
    if shift:
        v = (v + (1 << (shift - 1))) >> shift
    return np.clip(v, 0, 255).astype(np.uint8)


def rgba(full, ow, oh, rects, kind, pad=(0, 0, 0), canvas=None, stats=None, mutant=None):
    """full: (h, w, 4) uint8 -> (H', W', 4) uint8, alpha 255 wherever it is written"""
    (sx, sy, sw, sh), (dx, dy, dw, dh) = rects
    out = np.empty((oh, ow, 4), np.uint8) if canvas is None else canvas.copy()
    if canvas is None:
        out[:, :] = list(pad) + [255]
    win = np.ascontiguousarray(full[sy:sy + sh, sx:sx + sw, :3])
    out[dy:dy + dh, dx:dx + dw, :3] = resize(win, dw, dh, kind, stats, mutant)
    out[dy:dy + dh, dx:dx + dw, 3] = 255
    return out


def tensor(full, ow, oh, rects, kind, pad, dtype, scale, bias, bgr=False):
    """-> (3, H', W') bit patterns of the whole W' x H' output (mask with framing_ref.inside() for keep_outside)"""
    return tensor_out_ref.planes(rgba(full, ow, oh, rects, kind, pad), dtype, scale, bias, bgr)
