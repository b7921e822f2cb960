"""The shapes that the framed kernels are checked at, lane by lane on the CPU (test_sim_framed.py) and on the device
(test_gpu_framing.py), and the hazards that each of them must meet -- established here on the REFERENCE's side, from the
rectangles alone -- TEST INFRASTRUCTURE."""
import framing_ref as ref

QCIF, CIF = (176, 144), (352, 288)
# name -> (source size, output size, mode, source rectangle, destination rectangle)
CASES = {
    "qcif_window_odd": (QCIF, (130, 41), ref.WINDOW, (3, 5, 170, 131), (7, 3, 101, 33)),
    "qcif_window_thin": (QCIF, (12, 4), ref.WINDOW, (0, 0, 176, 144), (1, 1, 9, 2)),
    "qcif_one_pixel": (QCIF, (9, 6), ref.WINDOW, (175, 143, 1, 1), (2, 1, 5, 3)),
    "qcif_enlarging": (QCIF, (80, 55), ref.WINDOW, (10, 20, 30, 20), (5, 2, 70, 50)),
    "cif_window_300": (CIF, (65, 5), ref.WINDOW, (33, 7, 300, 200), (0, 0, 65, 4)),
    "cif_letterbox_224": (CIF, (224, 224), ref.LETTERBOX, (0, 0, 0, 0), (0, 0, 0, 0)),
    "cif_cover_224": (CIF, (224, 224), ref.COVER, (0, 0, 0, 0), (0, 0, 0, 0)),
    "cif_letterbox_65x5": (CIF, (65, 5), ref.LETTERBOX, (0, 0, 0, 0), (0, 0, 0, 0)),
    "cif_cover_65x5": (CIF, (65, 5), ref.COVER, (0, 0, 0, 0), (0, 0, 0, 0)),
}
ROWS_PER_BAND, COLS_PER_SEGMENT, CHUNK = 4, 64, 256
ALL_HAZARDS = {"mixed_segment", "pad_only_segment", "band_pad_above_and_below", "window_over_256_columns_odd_sx", "one_pixel_source",
               "enlarging", "full_width_partial_height", "full_height_partial_width", "dx_odd_dw_odd"}


def rects(name):
    (w, h), (ow, oh), mode, s, d = CASES[name]
    rc = ref.resolve(w, h, ow, oh, mode, s, d)
    assert rc is not None and not ref.whole(w, h, ow, oh, rc), name
    return rc


def hazards(name):
    """what the shape makes the kernels meet"""
    (w, h), (ow, oh), _, _, _ = CASES[name]
    (sx, sy, sw, sh), (dx, dy, dw, dh) = rects(name)
    out = set()
    for x0 in range(0, ow, COLS_PER_SEGMENT):
        cols = range(x0, min(x0 + COLS_PER_SEGMENT, ow))
        n_in = sum(1 for x in cols if dx <= x < dx + dw)
        if 0 < n_in < len(cols):
            out.add("mixed_segment")
        if n_in == 0:
            out.add("pad_only_segment")
        if n_in:
            # the source columns that the segment's columns of the rectangle cover
            xa, xb = max(x0, dx) - dx, min(cols[-1], dx + dw - 1) - dx
            first, last = sx + xa * sw // dw, sx + ((xb + 1) * sw - 1) // dw
            if last + 1 - (first & ~3) > CHUNK and sx % 2:
                out.add("window_over_256_columns_odd_sx")
    for y0 in range(0, oh, ROWS_PER_BAND):
        rows = range(y0, min(y0 + ROWS_PER_BAND, oh))
        if rows[0] < dy and rows[-1] >= dy + dh:
            out.add("band_pad_above_and_below")
    if sw == 1 and sh == 1:
        out.add("one_pixel_source")
    if dw > sw and dh > sh:
        out.add("enlarging")
    if dw == ow and dh < oh:
        out.add("full_width_partial_height")
    if dh == oh and dw < ow:
        out.add("full_height_partial_width")
    if dx % 2 and dw % 2 and dx + dw < ow:
        out.add("dx_odd_dw_odd")
    return out


def straddling_pairs(name, base, stride_c, stride_h):
    """16-bit elements at element index base + p*stride_c + Y*stride_h + X: (pairs across the left edge, pairs across the right
    edge) -- dwords that hold one element of the rectangle and one outside it, over the rectangle's rows and the three planes"""
    (_, _), (ow, oh), _, _, _ = CASES[name]
    _, (dx, dy, dw, dh) = rects(name)
    left = right = 0
    for p in range(3):
        for y in range(dy, dy + dh):
            row = base + p * stride_c + y * stride_h
            if dx > 0 and (row + dx - 1) % 2 == 0:
                left += 1
            if dx + dw < ow and (row + dx + dw - 1) % 2 == 0:
                right += 1
    return left, right
