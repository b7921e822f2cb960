"""numpy restatement of the resized deblocked-plane output under a filter (include/h263mi.h:
h263mi_batch_set_yuv_resize_filtered) -- TEST INFRASTRUCTURE.

Every plane is resampled on its own by filter_ref.resize (Pillow's two passes, restated) applied to one 8-bit channel: luma
w x h -> W' x H', Cb and Cr cw x ch -> cW' x cH', c* = ceil(* / 2), each axis with the taps of that plane's own sizes.
tests/test_plane_filter.py holds planes() to Image.fromarray(plane, "L").resize(...) of Pillow.  The placement is
yuv_layout_ref's for a W' x H' picture (yuv_resize_ref.place); the extent is yuv_resize_ref.extent, unchanged by the filter.

planes(y, cb, cr, ow, oh, kind, w, h, stats=None, mutant=None) -> (y', cb', cr') flat uint8 arrays
    stats (a dict, may be None): {"y": {"h": {"lo", "hi"}, "v": {...}}, "cb": ..., "cr": ...} of filter_ref.axis_pass
    mutant: None, "single" or "mask" as filter_ref.resize takes it
placements(ow, oh, fmt, n): the three placements the kernel is checked at
    -> {name: (pitch_y, pitch_c, (oy, ocb, ocr), given, base, bytes)}; given: the offset arrays are handed to the library (else
    they are the default placement, spelled out, and the library is given none)
"""
import numpy as np

import filter_ref
import yuv_layout_ref as lay
import yuv_resize_ref

I420, NV12 = lay.I420, lay.NV12
BILINEAR, BICUBIC = filter_ref.BILINEAR, filter_ref.BICUBIC
NAMES = ("y", "cb", "cr")


def planes(y, cb, cr, ow, oh, kind, w, h, stats=None, mutant=None):
    (cw, ch), (cow, coh) = lay.chroma_size(w, h), lay.chroma_size(ow, oh)
    out = []
    for name, p, (pw, ph), (pow_, poh) in zip(NAMES, (y, cb, cr), ((w, h), (cw, ch), (cw, ch)), ((ow, oh), (cow, coh), (cow, coh))):
        st = None if stats is None else stats.setdefault(name, {})
        out.append(filter_ref.resize(np.asarray(p, np.uint8).reshape(ph, pw), pow_, poh, kind, st, mutant).ravel())
    return tuple(out)


def place(canvas, pictures, ow, oh, fmt, pitch_y, pitch_c, oy, ocb, ocr, skip=()):
    return yuv_resize_ref.place(canvas, pictures, ow, oh, fmt, pitch_y, pitch_c, oy, ocb, ocr, skip=skip)


def placements(ow, oh, fmt, n):
    """tight: default placement at the rows' own lengths rounded up to 4 -- word stores;
    odd: pitches W' + 3 and cW' + 1 (NV12: 2 cW' + 1) made odd, every plane at an odd offset -- byte stores;
    shifted: pitches that are multiples of 4, every offset a multiple of 4, the whole placement on a base that is 1 modulo 4 --
    byte stores again (the base counts).  `base`: where d_deblocked starts in the canvas; `bytes`: the canvas.  Every placement
    is one that h263mi_yuv_resize_extent accepts (rows do not cross their pitch boundary, planes follow one another)"""
    ry, rc = lay.row_bytes(ow, fmt)
    coh = (oh + 1) // 2

    def explicit(py, pc, first, ok):
        """the planes one behind the other, each at the first offset that `ok` accepts and whose rows stay inside their pitch"""
        def fit(at, pitch, row):
            while not (ok(at) and at % pitch + row <= pitch):
                at += 1
            return at
        oy, ocb, ocr = [], [], ([] if fmt != NV12 else None)
        at = first
        for _ in range(n):
            oy.append(fit(at, py, ry))
            at = oy[-1] + oh * py
            ocb.append(fit(at, pc, rc))
            at = ocb[-1] + coh * pc
            if fmt != NV12:
                ocr.append(fit(at, pc, rc))
                at = ocr[-1] + coh * pc
        return oy, ocb, ocr, at

    out = {}
    py, pc = (ry + 3) // 4 * 4, (rc + 3) // 4 * 4
    oy, ocb, ocr = lay.default_offsets(n, ow, oh, fmt, py, pc)
    out["tight"] = (py, pc, (oy, ocb, ocr), False, 0, n * lay.picture_bytes(ow, oh, fmt, py, pc))
    py, pc = (ow + 3) | 1, (rc + 1) | 1
    oy, ocb, ocr, end = explicit(py, pc, 1, lambda o: o % 2 == 1)
    out["odd"] = (py, pc, (oy, ocb, ocr), True, 0, end + 8)
    py, pc = (ry + 3) // 4 * 4 + 4, (rc + 3) // 4 * 4 + 8
    oy, ocb, ocr, end = explicit(py, pc, 0, lambda o: o % 4 == 0)
    out["shifted"] = (py, pc, (oy, ocb, ocr), True, 1, 1 + end + 8)
    return out
