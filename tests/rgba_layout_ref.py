"""numpy restatement of the RGBA output layout (include/h263mi.h: h263mi_rgba_layout) -- TEST INFRASTRUCTURE.

box_average: the full-size RGBA P (what h263mi_render_rgba returns) -> W' x H' = ceil(w/f) x ceil(h/f), f = 2^scale_log2;
out[Y][X][c] = (S + n/2) // n over the n pixels of the f x f box at (fX, fY) that lie inside the picture, alpha 255.
place: the pictures into a canvas, H' rows of 4W' bytes, row_pitch apart, picture s at offsets[s].
extent: h263mi_rgba_layout_extent restated (None where the layout is refused).
Pinned by tests/golden/rgba_layout_known_answers.json (tests/test_rgba_layout.py).
"""
import numpy as np


def out_size(w, h, scale_log2):
    f = 1 << scale_log2
    return (w + f - 1) // f, (h + f - 1) // f


def box_average(rgba, w, h, scale_log2):
    """rgba: w*h*4 bytes (or an (h, w, 4) array) -> (H', W', 4) uint8"""
    p = np.asarray(rgba, np.uint8).reshape(h, w, 4)
    f = 1 << scale_log2
    ow, oh = out_size(w, h, scale_log2)
    pad = np.zeros((oh * f, ow * f, 3), np.int64)
    pad[:h, :w] = p[:, :, :3]
    inside = np.zeros((oh * f, ow * f), np.int64)
    inside[:h, :w] = 1
    s = pad.reshape(oh, f, ow, f, 3).sum(axis=(1, 3))
    n = inside.reshape(oh, f, ow, f).sum(axis=(1, 3))[:, :, None]
    out = np.full((oh, ow, 4), 255, np.uint8)
    out[:, :, :3] = (s + n // 2) // n
    return out


def default_pitch(w, scale_log2):
    return 4 * out_size(w, 1, scale_log2)[0]


def default_offsets(n, w, h, scale_log2, row_pitch=0):
    ow, oh = out_size(w, h, scale_log2)
    pitch = row_pitch or 4 * ow
    return [s * oh * pitch for s in range(n)]


def place(canvas, pictures, row_pitch, offsets):
    """pictures: (H', W', 4) arrays; writes each into the flat uint8 canvas, row by row"""
    for pic, off in zip(pictures, offsets):
        oh, ow = pic.shape[:2]
        for r in range(oh):
            canvas[off + r * row_pitch: off + r * row_pitch + 4 * ow] = pic[r].ravel()
    return canvas


def rect_mask(canvas_bytes, w, h, scale_log2, row_pitch, offsets):
    """True where some picture of the layout writes"""
    ow, oh = out_size(w, h, scale_log2)
    m = np.zeros(canvas_bytes, bool)
    for off in offsets:
        for r in range(oh):
            m[off + r * row_pitch: off + r * row_pitch + 4 * ow] = True
    return m


def extent(n, w, h, scale_log2=0, row_pitch=0, offsets=None, reserved=0):
    """(W', H', bytes) of h263mi_rgba_layout_extent, or None where it answers H263MI_ERR_INVALID_ARGUMENT"""
    if n == 0 or w == 0 or h == 0 or scale_log2 > 2 or reserved:
        return None
    ow, oh = out_size(w, h, scale_log2)
    row = 4 * ow
    pitch = row_pitch or row
    if pitch < row or pitch % 4:
        return None
    span = (oh - 1) * pitch + row
    if span >= 1 << 32:
        return None
    if offsets is None:
        return ow, oh, (n - 1) * oh * pitch + span
    rects = []
    for o in offsets:
        if o % 4 or o % pitch + row > pitch:
            return None
        rects.append((o // pitch, o % pitch))
    for i in range(n):
        for j in range(i + 1, n):
            (ri, ci), (rj, cj) = rects[i], rects[j]
            if ri < rj + oh and rj < ri + oh and ci < cj + row and cj < ci + row:
                return None
    return ow, oh, max(o + span for o in offsets)
