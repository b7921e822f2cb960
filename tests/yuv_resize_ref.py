"""numpy restatement of the resized deblocked-plane output (include/h263mi.h: h263mi_yuv_resize) -- TEST INFRASTRUCTURE.

Every plane is resized on its own by the area average of h263mi_rgba_resize applied to one 8-bit channel: for a plane P of
pw x ph and an output of pw' x ph'
    out[Y][X] = (sum_j sum_i oy(Y,j) ox(X,i) P[j][i] + floor(pw*ph/2)) // (pw*ph)
with the weights of rgba_resize_ref.spans.  Luma: (w, h, W', H'); Cb and Cr: (cw, ch, cW', cH'), c* = ceil(* / 2).  The placement
is yuv_layout_ref's for a W' x H' picture.  extent: h263mi_yuv_resize_extent restated (None where the resize is refused).
Pinned by tests/golden/yuv_resize_known_answers.json (tests/test_yuv_resize.py).
"""
import numpy as np

import rgba_resize_ref
import yuv_layout_ref

I420, NV12 = yuv_layout_ref.I420, yuv_layout_ref.NV12


def resize_plane(p, pw, ph, ow, oh):
    """p: pw*ph samples (flat or (ph, pw)) -> (oh, ow) uint8"""
    p = np.asarray(p, np.uint8).reshape(ph, pw).astype(np.int64)
    (iy, wy), (ix, wx) = rgba_resize_ref.spans(ph, oh), rgba_resize_ref.spans(pw, ow)
    t = np.zeros((oh, pw), np.int64)
    for k in range(iy.shape[1]):
        t += wy[:, k, None] * p[iy[:, k]]
    s = np.zeros((oh, ow), np.int64)
    for k in range(ix.shape[1]):
        s += wx[None, :, k] * t[:, ix[:, k]]
    d = pw * ph
    return ((s + d // 2) // d).astype(np.uint8)


def resize_planes(planes, w, h, ow, oh):
    """(y, cb, cr) of a w x h picture -> (y, cb, cr) of the ow x oh one, flat uint8 arrays"""
    (cw, ch), (cow, coh) = yuv_layout_ref.chroma_size(w, h), yuv_layout_ref.chroma_size(ow, oh)
    y, cb, cr = planes
    return (resize_plane(y, w, h, ow, oh).ravel(), resize_plane(cb, cw, ch, cow, coh).ravel(),
            resize_plane(cr, cw, ch, cow, coh).ravel())


def place(canvas, pictures, ow, oh, fmt, pitch_y, pitch_c, oy, ocb, ocr, skip=()):
    """resized pictures (resize_planes) into the canvas: yuv_layout_ref.place for an ow x oh picture"""
    return yuv_layout_ref.place(canvas, pictures, ow, oh, fmt, pitch_y, pitch_c, oy, ocb, ocr, skip=skip)


def _layout_extent(n, w, h, fmt, pitch_y, pitch_c, oy, ocb, ocr):
    """h263mi_yuv_layout_extent restated: bytes, or None where the layout is refused"""
    if n == 0 or w == 0 or h == 0 or fmt not in (I420, NV12):
        return None
    nv12 = fmt == NV12
    cw, ch = yuv_layout_ref.chroma_size(w, h)
    ry, rc = yuv_layout_ref.row_bytes(w, fmt)
    py, pc = pitch_y or ry, pitch_c or rc
    if py < ry or pc < rc:
        return None
    if (h > 1 and py >= 1 << 32) or (ch > 1 and pc >= 1 << 32):
        return None
    span_y, span_c = (h - 1) * py + ry, (ch - 1) * pc + rc
    if span_y >= 1 << 32 or span_c >= 1 << 32:
        return None
    if nv12 and ocr is not None:
        return None
    given = sum(o is not None for o in (oy, ocb, ocr))
    if given not in (0, 2 if nv12 else 3):
        return None
    if given == 0:
        total = n * yuv_layout_ref.picture_bytes(w, h, fmt, py, pc)
        return total if total < 1 << 64 else None
    rects = {False: [], True: []}
    spans = []
    total = 0
    for s in range(n):
        planes = [(int(oy[s]), py, ry, h, span_y, False), (int(ocb[s]), pc, rc, ch, span_c, True)]
        if not nv12:
            planes.append((int(ocr[s]), pc, rc, ch, span_c, True))
        for o, pitch, row, rows, span, chroma in planes:
            if o % pitch + row > pitch or o + span >= 1 << 64:
                return None
            total = max(total, o + span)
            rects[chroma].append((o // pitch, o % pitch, rows, row))
            spans.append((o, o + span, chroma))

    def intersect(rs):
        for i in range(len(rs)):
            for j in range(i + 1, len(rs)):
                a, b = rs[i], rs[j]
                if a[0] < b[0] + b[2] and b[0] < a[0] + a[2] and a[1] < b[1] + b[3] and b[1] < a[1] + a[3]:
                    return True
        return False
    if py == pc:
        if intersect(rects[False] + rects[True]):
            return None
    else:
        if intersect(rects[False]) or intersect(rects[True]):
            return None
        for lo, hi, chroma in spans:
            for lo2, hi2, chroma2 in spans:
                if chroma != chroma2 and lo < hi2 and lo2 < hi:
                    return None
    return total


def extent(n, ow, oh, fmt=I420, pitch_y=0, pitch_c=0, oy=None, ocb=None, ocr=None, reserved=0):
    """bytes of h263mi_yuv_resize_extent, or None where it answers H263MI_ERR_INVALID_ARGUMENT"""
    if n == 0 or ow == 0 or oh == 0 or reserved:
        return None
    return _layout_extent(n, ow, oh, fmt, pitch_y, pitch_c, oy, ocb, ocr)
