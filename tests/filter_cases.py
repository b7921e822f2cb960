"""The shapes that the filter kernels (k_rgba_filter, k_tensor_filter) are checked at, lane by lane on the CPU
(test_sim_filter.py) and on the device (test_gpu_filter.py), and the hazards that each of them must meet -- established here on
the REFERENCE's side, from the tap tables and from filter_ref's own arithmetic on the picture -- TEST INFRASTRUCTURE."""
import numpy as np

import filter_ref as ref
import framing_cases as fc
import framing_ref as fref

QCIF, CIF = fc.QCIF, fc.CIF
_NONE = (0, 0, 0, 0)
# name -> (source size, output size, mode, source rectangle, destination rectangle)
CASES = {
    "qcif_224": (QCIF, (224, 224), fref.STRETCH, _NONE, _NONE),                 # enlarging
    "cif_50x37": (CIF, (50, 37), fref.STRETCH, _NONE, _NONE),
    "cif_1x1": (CIF, (1, 1), fref.STRETCH, _NONE, _NONE),                       # taps over every column and every row
    "qcif_65x5": (QCIF, (65, 5), fref.STRETCH, _NONE, _NONE),                   # a last segment of 1 column, a last band of 1 row
    "qcif_176x97": (QCIF, (176, 97), fref.STRETCH, _NONE, _NONE),               # the horizontal pass is skipped
    "qcif_129x144": (QCIF, (129, 144), fref.STRETCH, _NONE, _NONE),             # the vertical pass is skipped
    "cif_letterbox_224": fc.CASES["cif_letterbox_224"],
    "cif_cover_224": fc.CASES["cif_cover_224"],
    "cif_window_300": fc.CASES["cif_window_300"],                               # odd sx, more than 256 source columns
    "qcif_one_pixel": fc.CASES["qcif_one_pixel"],
    "qcif_enlarging": fc.CASES["qcif_enlarging"],
}
KINDS = [ref.BILINEAR, ref.BICUBIC]
KIND_IDS = ["bilinear", "bicubic"]
ROWS_PER_BAND, COLS_PER_SEGMENT, CHUNK = 4, 64, 256
GEOMETRY_HAZARDS = {"taps_cut_left", "taps_cut_right", "taps_cut_top", "taps_cut_bottom", "shared_tap_window", "horizontal_skipped",
                    "vertical_skipped", "taps_over_256_columns", "last_segment_one_column", "last_band_one_row", "odd_sx",
                    "one_pixel_source", "framed"}
CONTENT_HAZARDS = {"h_clamp_0", "h_clamp_255", "v_clamp_0", "v_clamp_255", "single_rounding_differs", "mask_differs"}
ALL_HAZARDS = GEOMETRY_HAZARDS | CONTENT_HAZARDS


def rects(name):
    (w, h), (ow, oh), mode, s, d = CASES[name]
    rc = fref.resolve(w, h, ow, oh, mode, s, d)
    assert rc is not None, name
    return rc


def picture(size, index):
    """a source picture for the CPU tests, (h, w, 4) uint8, alpha 255: noise over flat blocks of 0 and 255 with hard edges, so a
    cubic's negative lobes leave 0..255 on both sides in both passes"""
    w, h = size
    rng = np.random.default_rng(w * 7 + h * 13 + index)
    blocks = rng.integers(0, 2, ((h + 7) // 8, (w + 5) // 6, 3)) * 255
    pic = np.repeat(np.repeat(blocks, 8, axis=0), 6, axis=1)[:h, :w]
    noise = rng.integers(-20, 21, (h, w, 3))
    pic = np.clip(pic + noise * (rng.random((h, w, 1)) < 0.5), 0, 255)
    return np.concatenate([pic, np.full((h, w, 1), 255)], axis=2).astype(np.uint8)


def _cut(kind, n_in, n_out):
    """(some tap window is cut at the low edge, at the high edge): the windows as the definition places them before it clamps"""
    scale = n_in / n_out
    support = ref.SUPPORT[kind] * max(scale, 1.0)
    lo = hi = False
    for X in range(n_out):
        center = (X + 0.5) * scale
        lo = lo or center - support + 0.5 <= -1.0
        hi = hi or int(center + support + 0.5) > n_in
    return lo, hi


def geometry_hazards(name, kind):
    (w, h), (ow, oh), _, _, _ = CASES[name]
    (sx, sy, sw, sh), (dx, dy, dw, dh) = rects(name)
    out = set()
    (_, fx, cx, _), (_, fy, cy, _) = ref.taps(kind, sw, dw), ref.taps(kind, sh, dh)
    if dw != sw:
        lo, hi = _cut(kind, sw, dw)
        out |= ({"taps_cut_left"} if lo else set()) | ({"taps_cut_right"} if hi else set())
        if any(fx[X] == fx[X + 1] and cx[X] == cx[X + 1] for X in range(dw - 1)):
            out.add("shared_tap_window")
    else:
        out.add("horizontal_skipped")
    if dh != sh:
        lo, hi = _cut(kind, sh, dh)
        out |= ({"taps_cut_top"} if lo else set()) | ({"taps_cut_bottom"} if hi else set())
    else:
        out.add("vertical_skipped")
    for x0 in range(dx - dx % COLS_PER_SEGMENT, dx + dw, COLS_PER_SEGMENT):
        xa, xb = max(x0, dx) - dx, min(x0 + COLS_PER_SEGMENT, dx + dw) - 1 - dx
        if dw != sw and fx[xb] + cx[xb] - ((sx + fx[xa]) & ~3) + sx > CHUNK:
            out.add("taps_over_256_columns")
    if ow % COLS_PER_SEGMENT == 1:
        out.add("last_segment_one_column")
    if oh % ROWS_PER_BAND == 1:
        out.add("last_band_one_row")
    if sx % 2:
        out.add("odd_sx")
    if sw == 1 and sh == 1:
        out.add("one_pixel_source")
    if not fref.whole(w, h, ow, oh, rects(name)):
        out.add("framed")
    return out


def content_hazards(name, kind, full):
    """what the picture `full` (h, w, 4) makes the arithmetic meet inside the destination rectangle"""
    (_, _), (ow, oh), _, _, _ = CASES[name]
    rc = rects(name)
    stats = {}
    two = ref.rgba(full, ow, oh, rc, kind, stats=stats)
    out = set()
    for axis in "hv":
        if stats.get(axis, {}).get("lo"):
            out.add(axis + "_clamp_0")
        if stats.get(axis, {}).get("hi"):
            out.add(axis + "_clamp_255")
    if (ref.rgba(full, ow, oh, rc, kind, mutant="single") != two).any():
        out.add("single_rounding_differs")
    if (ref.rgba(full, ow, oh, rc, kind, mutant="mask") != two).any():
        out.add("mask_differs")
    return out
