"""The shapes that k_plane_filter is checked at, lane by lane on the CPU (test_sim_plane_filter.py) and on the device
(test_gpu_plane_filter.py), and the hazards that each of them must meet -- established here on the REFERENCE's side, from the tap
tables, the kernel's published constants and plane_filter_ref's own arithmetic on the picture -- TEST INFRASTRUCTURE."""
import numpy as np

import filter_ref as flt
import plane_filter_ref as ref
import recgen
import yuv_layout_ref as lay
from oracle import oracle as orc

QCIF, CIF, ODD, WIDE = (176, 144), (352, 288), (75, 51), (600, 16)
SIZES = (QCIF, CIF, ODD)         # what the device tests decode
STRENGTH = 7                     # the deblocking strength of every picture the cases are checked with
# name -> (source size, output size)
CASES = {
    "qcif_224": (QCIF, (224, 224)),          # enlarging; clamps in both passes of all three planes
    "cif_50x37": (CIF, (50, 37)),            # shrinking; odd W', H' (cW' 25, cH' 19)
    "cif_1x1": (CIF, (1, 1)),                # taps over every column and row; more than one chunk; rows beyond the LDS cap
    "qcif_257x5": (QCIF, (257, 5)),          # a last luma segment of one column; a last band of one row; cH' = 3
    "qcif_176x97": (QCIF, (176, 97)),        # the horizontal pass skipped in every plane
    "qcif_129x144": (QCIF, (129, 144)),      # the vertical pass skipped in every plane
    "qcif_175x144": (QCIF, (175, 144)),      # luma's horizontal pass runs, chroma's is skipped (cW' = 88 = cw)
    "qcif_176x143": (QCIF, (176, 143)),      # luma's vertical pass runs; chroma is copied
    "odd_40x30": (ODD, (40, 30)),            # cw 38, ch 26: no 16-byte-aligned chroma rows
    "odd_224": (ODD, (224, 224)),            # enlarging an odd source
    "qcif_25x144": (QCIF, (25, 144)),        # bilinear: luma coefficient rows of 17, just beyond the LDS cap, chroma rows of 15, just within
    "wide_5x3": (WIDE, (5, 3)),              # chroma taps over more than one chunk (cw = 300): CPU only, the device tests stop at CIF
    "identity": (QCIF, QCIF),                # the full-size layout path
}
CPU_ONLY = {"wide_5x3"}
GPU_CASES = [name for name in CASES if name not in CPU_ONLY]
KINDS = [flt.BILINEAR, flt.BICUBIC]
KIND_IDS = ["bilinear", "bicubic"]
# plane_filter_kernel.inl: PFILTER_ROWS, PLANE_OUT, PFILTER_CHUNK, PFILTER_SRC, PFILTER_LDS_TAPS
ROWS_PER_BAND, COLS_PER_SEGMENT, CHUNK, SRC, LDS_TAPS = 4, 256, 256, 16, 16
PLANES = ("y", "c")
GEOMETRY_HAZARDS = ({p + "_taps_cut_" + e for p in PLANES for e in ("left", "right", "top", "bottom")} |
                    {p + "_shared_tap_window" for p in PLANES} |
                    {p + "_taps_over_one_chunk" for p in PLANES} |
                    {p + "_coeff_rows_beyond_lds_cap" for p in PLANES} | {p + "_coeff_rows_in_lds" for p in PLANES} |
                    {"horizontal_skipped", "vertical_skipped", "chroma_horizontal_skipped_only", "chroma_vertical_skipped_only",
                     "chroma_wholly_skipped", "odd_source", "odd_output", "unaligned_chroma_rows", "last_segment_one_column",
                     "last_band_one_row", "chroma_last_band_short", "luma_beyond_lds_cap_chroma_within", "full_size"})
CONTENT_HAZARDS = ({p + "_" + a + "_clamp_" + v for p in PLANES for a in "hv" for v in ("0", "255")} |
                   {p + "_single_rounding_differs" for p in PLANES} | {p + "_mask_differs" for p in PLANES})
ALL_HAZARDS = GEOMETRY_HAZARDS | CONTENT_HAZARDS

_pictures = {}


def picture(size, index=0, strength=STRENGTH):
    """(y, cb, cr) flat uint8: recgen.intra_picture(w, h, seed=w + 5 + index) decoded by the oracle, deblocked"""
    key = (size, index, strength)
    if key not in _pictures:
        w, h = size
        mbs, co = recgen.intra_picture(w, h, seed=w + 5 + index)
        rc, planes = orc.decode_picture(w, h, mbs, co, None)
        assert rc == 0
        cw = (w + 1) // 2
        if strength:
            planes = tuple(orc.deblock(p, pw, strength) for p, pw in zip(planes, (w, cw, cw)))
        _pictures[key] = tuple(np.asarray(p, np.uint8).ravel() for p in planes)
    return _pictures[key]


def records(size, index=0):
    """the macroblock records and coefficients of picture(size, index)"""
    return recgen.intra_picture(size[0], size[1], seed=size[0] + 5 + index)


def _cut(kind, n_in, n_out):
    """(some tap window is cut at the low edge, at the high edge): the windows as the definition places them before it clamps"""
    scale = n_in / n_out
    support = flt.SUPPORT[kind] * max(scale, 1.0)
    lo = hi = False
    for X in range(n_out):
        center = (X + 0.5) * scale
        lo = lo or center - support + 0.5 <= -1.0
        hi = hi or int(center + support + 0.5) > n_in
    return lo, hi


def _plane_geometry(p, kind, pw, ph, ow, oh):
    out = set()
    if ow != pw:
        ks, fx, cx, _ = flt.taps(kind, pw, ow)
        lo, hi = _cut(kind, pw, ow)
        out |= ({p + "_taps_cut_left"} if lo else set()) | ({p + "_taps_cut_right"} if hi else set())
        if any(fx[X] == fx[X + 1] and cx[X] == cx[X + 1] for X in range(ow - 1)):
            out.add(p + "_shared_tap_window")
        out.add(p + ("_coeff_rows_beyond_lds_cap" if ks > LDS_TAPS else "_coeff_rows_in_lds"))
        for x0 in range(0, ow, COLS_PER_SEGMENT):
            x1 = min(x0 + COLS_PER_SEGMENT, ow) - 1
            if fx[x1] + cx[x1] - (fx[x0] & ~(SRC - 1)) > CHUNK:
                out.add(p + "_taps_over_one_chunk")
    if oh != ph:
        lo, hi = _cut(kind, ph, oh)
        out |= ({p + "_taps_cut_top"} if lo else set()) | ({p + "_taps_cut_bottom"} if hi else set())
    return out


def geometry_hazards(name, kind):
    (w, h), (ow, oh) = CASES[name]
    (cw, ch), (cow, coh) = lay.chroma_size(w, h), lay.chroma_size(ow, oh)
    out = _plane_geometry("y", kind, w, h, ow, oh) | _plane_geometry("c", kind, cw, ch, cow, coh)
    if (ow, oh) == (w, h):
        return out | {"full_size"}
    if {"y_coeff_rows_beyond_lds_cap", "c_coeff_rows_in_lds"} <= out:
        out.add("luma_beyond_lds_cap_chroma_within")
    if ow == w and cow == cw:
        out.add("horizontal_skipped")
    if oh == h and coh == ch:
        out.add("vertical_skipped")
    if ow != w and cow == cw:
        out.add("chroma_horizontal_skipped_only")
    if oh != h and coh == ch:
        out.add("chroma_vertical_skipped_only")
    if cow == cw and coh == ch:
        out.add("chroma_wholly_skipped")
    if w % 2 or h % 2:
        out.add("odd_source")
    if ow % 2 and oh % 2:
        out.add("odd_output")
    if cw % 16:
        out.add("unaligned_chroma_rows")
    if ow % COLS_PER_SEGMENT == 1:
        out.add("last_segment_one_column")
    if oh % ROWS_PER_BAND == 1:
        out.add("last_band_one_row")
    if coh % ROWS_PER_BAND:
        out.add("chroma_last_band_short")
    return out


_content = {}


def content_hazards(name, kind, index=0):
    """what picture(size, index) makes the arithmetic meet, per plane kind (y; c: Cb or Cr)"""
    key = (name, kind, index)
    if key in _content:
        return _content[key]
    (w, h), (ow, oh) = CASES[name]
    pic = picture((w, h), index)
    stats = {}
    two = ref.planes(*pic, ow, oh, kind, w, h, stats=stats)
    single = ref.planes(*pic, ow, oh, kind, w, h, mutant="single")
    mask = ref.planes(*pic, ow, oh, kind, w, h, mutant="mask")
    out = set()
    for k, pname in enumerate(ref.NAMES):
        p = "y" if pname == "y" else "c"
        for axis in "hv":
            if stats[pname].get(axis, {}).get("lo"):
                out.add(p + "_" + axis + "_clamp_0")
            if stats[pname].get(axis, {}).get("hi"):
                out.add(p + "_" + axis + "_clamp_255")
        if (single[k] != two[k]).any():
            out.add(p + "_single_rounding_differs")
        if (mask[k] != two[k]).any():
            out.add(p + "_mask_differs")
    _content[key] = out
    return out


_want = {}


def want(name, kind, index=0, mutant=None):
    """the resampled planes of picture(size, index), made once"""
    key = (name, kind, index, mutant)
    if key not in _want:
        (w, h), (ow, oh) = CASES[name]
        _want[key] = ref.planes(*picture((w, h), index), ow, oh, kind, w, h, mutant=mutant)
    return _want[key]
