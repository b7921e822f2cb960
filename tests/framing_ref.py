"""Restatement of the framing of a resized output (include/h263mi.h: h263mi_framing) in Python integers and numpy -- TEST
INFRASTRUCTURE.

resolve(w, h, ow, oh, mode, ...): h263mi_framing_resolve -> ((sx, sy, sw, sh), (dx, dy, dw, dh)), or None where it answers
    H263MI_ERR_INVALID_ARGUMENT.  rnd(a, b) = (2a + b) div 2b, nothing wraps.
rgba(full, ow, oh, rects, pad, canvas): the W' x H' RGBA: rgba_resize_ref.resize of the source window, pasted at (dx, dy) into
    a canvas of the pad colour (alpha 255) -- or into `canvas` (what keep_outside leaves untouched).
tensor(full, ow, oh, rects, pad, dtype, scale, bias, bgr): tensor_out_ref.planes of rgba(...): the pad colour is a `u` like any
    other.  inside(rects, oh, ow): the (H', W') mask of the destination rectangle.
Pinned by tests/golden/framing_known_answers.json (tests/test_framing.py).
"""
import numpy as np

import rgba_resize_ref
import tensor_out_ref

STRETCH, LETTERBOX, COVER, WINDOW = 0, 1, 2, 3
MODES = {"stretch": STRETCH, "letterbox": LETTERBOX, "cover": COVER, "window": WINDOW}


def rnd(a, b):
    return (2 * a + b) // (2 * b)


def clamp(v, lo, hi):
    return max(lo, min(hi, v))


def resolve(w, h, ow, oh, mode=STRETCH, src=(0, 0, 0, 0), dst=(0, 0, 0, 0), keep_outside=0, reserved=(0, 0, 0)):
    if min(w, h, ow, oh) < 1 or mode > WINDOW or keep_outside > 1 or any(reserved):
        return None
    if mode != WINDOW and (any(src) or any(dst)):
        return None
    s, d = (0, 0, w, h), (0, 0, ow, oh)
    if mode == LETTERBOX:
        if w * oh >= h * ow:
            dw, dh = ow, clamp(rnd(h * ow, w), 1, oh)
        else:
            dw, dh = clamp(rnd(w * oh, h), 1, ow), oh
        d = ((ow - dw) // 2, (oh - dh) // 2, dw, dh)
    elif mode == COVER:
        if w * oh >= h * ow:
            sw, sh = clamp(rnd(h * ow, oh), 1, w), h
        else:
            sw, sh = w, clamp(rnd(w * oh, ow), 1, h)
        s = ((w - sw) // 2, (h - sh) // 2, sw, sh)
    elif mode == WINDOW:
        s, d = tuple(src), tuple(dst)
        if min(s[2], s[3], d[2], d[3]) < 1 or s[0] + s[2] > w or s[1] + s[3] > h or d[0] + d[2] > ow or d[1] + d[3] > oh:
            return None
    return s, d


def whole(w, h, ow, oh, rects):
    return rects == ((0, 0, w, h), (0, 0, ow, oh))


def inside(rects, oh, ow):
    dx, dy, dw, dh = rects[1]
    m = np.zeros((oh, ow), bool)
    m[dy:dy + dh, dx:dx + dw] = True
    return m


def rgba(full, ow, oh, rects, pad=(0, 0, 0), canvas=None):
    """full: (h, w, 4) uint8 -> (H', W', 4) uint8"""
    (sx, sy, sw, sh), (dx, dy, dw, dh) = rects
    out = np.empty((oh, ow, 4), np.uint8) if canvas is None else canvas.copy()
    if canvas is None:
        out[:, :] = list(pad) + [255]
    win = np.ascontiguousarray(full[sy:sy + sh, sx:sx + sw])
    out[dy:dy + dh, dx:dx + dw] = rgba_resize_ref.resize(win, sw, sh, dw, dh)
    return out


def tensor(full, ow, oh, rects, pad, dtype, scale, bias, bgr=False):
    """-> (3, H', W') bit patterns of the whole W' x H' output (mask with inside() for keep_outside)"""
    return tensor_out_ref.planes(rgba(full, ow, oh, rects, pad), dtype, scale, bias, bgr)
