"""numpy restatement of the deblocked-plane output layout (include/h263mi.h: h263mi_yuv_layout) -- TEST INFRASTRUCTURE.

A picture is (y, cb, cr): flat uint8 arrays of w*h, cw*ch, cw*ch samples, cw = ceil(w/2), ch = ceil(h/2).  I420 keeps the
three planes; NV12 keeps Y and one plane of ch rows of cw interleaved (Cb, Cr) pairs.  Luma rows lie pitch_y bytes apart,
chroma rows pitch_c; stream s's planes start at offsets (oy[s], ocb[s], ocr[s]) -- ocr is None for NV12.
"""
import numpy as np

I420, NV12 = 0, 1


def chroma_size(w, h):
    return (w + 1) // 2, (h + 1) // 2


def row_bytes(w, fmt):
    """(bytes of a luma row, bytes of a chroma row)"""
    cw = (w + 1) // 2
    return w, (2 * cw if fmt == NV12 else cw)


def pitches(w, fmt, pitch_y=0, pitch_c=0):
    ry, rc = row_bytes(w, fmt)
    return pitch_y or ry, pitch_c or rc


def interleave(cb, cr, w, h):
    """-> (ch, 2 cw) array of Cb,Cr pairs"""
    cw, ch = chroma_size(w, h)
    out = np.empty((ch, 2 * cw), np.uint8)
    out[:, 0::2] = np.asarray(cb, np.uint8).reshape(ch, cw)
    out[:, 1::2] = np.asarray(cr, np.uint8).reshape(ch, cw)
    return out


def picture_bytes(w, h, fmt, pitch_y=0, pitch_c=0):
    """P of the default placement: h*pitch_y + k*ch*pitch_c"""
    py, pc = pitches(w, fmt, pitch_y, pitch_c)
    ch = (h + 1) // 2
    return h * py + (1 if fmt == NV12 else 2) * ch * pc


def default_offsets(n, w, h, fmt, pitch_y=0, pitch_c=0):
    """-> (oy, ocb, ocr) lists (ocr None for NV12) of the default placement"""
    py, pc = pitches(w, fmt, pitch_y, pitch_c)
    ch = (h + 1) // 2
    P = picture_bytes(w, h, fmt, pitch_y, pitch_c)
    oy = [s * P for s in range(n)]
    ocb = [s * P + h * py for s in range(n)]
    ocr = None if fmt == NV12 else [s * P + h * py + ch * pc for s in range(n)]
    return oy, ocb, ocr


def planes_of(picture, w, h, fmt):
    """the 2-D byte arrays a picture is stored as: [Y, Cb, Cr] or [Y, CbCr]"""
    cw, ch = chroma_size(w, h)
    y, cb, cr = (np.asarray(p, np.uint8) for p in picture)
    if fmt == NV12:
        return [y.reshape(h, w), interleave(cb, cr, w, h)]
    return [y.reshape(h, w), cb.reshape(ch, cw), cr.reshape(ch, cw)]


def _rects(n, w, h, fmt, pitch_y, pitch_c, oy, ocb, ocr):
    """[(stream, plane index, offset, pitch, rows, row bytes)]"""
    py, pc = pitches(w, fmt, pitch_y, pitch_c)
    ry, rc = row_bytes(w, fmt)
    ch = (h + 1) // 2
    out = []
    for s in range(n):
        out.append((s, 0, int(oy[s]), py, h, ry))
        out.append((s, 1, int(ocb[s]), pc, ch, rc))
        if fmt != NV12:
            out.append((s, 2, int(ocr[s]), pc, ch, rc))
    return out


def place(canvas, pictures, w, h, fmt, pitch_y, pitch_c, oy, ocb, ocr, skip=()):
    """writes each picture's planes into the flat uint8 canvas, row by row; streams in `skip` are left out"""
    n = len(pictures)
    stored = [planes_of(p, w, h, fmt) if s not in skip else None for s, p in enumerate(pictures)]
    for s, k, off, pitch, rows, rb in _rects(n, w, h, fmt, pitch_y, pitch_c, oy, ocb, ocr):
        if stored[s] is None:
            continue
        for r in range(rows):
            canvas[off + r * pitch: off + r * pitch + rb] = stored[s][k][r]
    return canvas


def rect_mask(canvas_bytes, n, w, h, fmt, pitch_y, pitch_c, oy, ocb, ocr):
    """True where some plane of the layout lies"""
    m = np.zeros(canvas_bytes, bool)
    for s, k, off, pitch, rows, rb in _rects(n, w, h, fmt, pitch_y, pitch_c, oy, ocb, ocr):
        for r in range(rows):
            m[off + r * pitch: off + r * pitch + rb] = True
    return m


def span_end(n, w, h, fmt, pitch_y, pitch_c, oy, ocb, ocr):
    """the byte behind the last byte any plane occupies"""
    return max(off + (rows - 1) * pitch + rb for _, _, off, pitch, rows, rb in _rects(n, w, h, fmt, pitch_y, pitch_c, oy, ocb, ocr))
