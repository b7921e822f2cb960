"""The ROI tables that k_roi_tensor is checked at, lane by lane on the CPU (test_sim_roi.py) and on the device
(test_gpu_roi.py), and the hazards that each of them must meet -- established here on the REFERENCE's side, from the tables and
the placements alone -- TEST INFRASTRUCTURE."""
import numpy as np

import roi_ref as ref
import tensor_out_ref as tref

QCIF, CIF, ODD = (176, 144), (352, 288), (178, 50)            # (ODD: a width that 4 does not divide -- the byte-load path)
ROWS_PER_BAND, COLS_PER_SEGMENT, CHUNK = 4, 64, 256

# name -> (picture size, pictures, "random" | "white", (W', H'), [(picture, x, y, w, h[, reserved]), ...])
TABLES = {
    "qcif_65x5": (QCIF, 3, "random", (65, 5), [
        (2, 175, 143, 1, 1),                                  # one pixel: the last pixel of the last picture
        (2, 10, 20, 30, 20),                                  # w < W'
        (1, 3, 5, 170, 131),
        (1, 0, 0, 100, 100), (1, 50, 44, 100, 100),           # two that overlap
        (0, 0, 0, 176, 144),
        (0, 0, 0, 10, 10, 1),                                 # reserved set
        (3, 0, 0, 10, 10), (0xFFFFFFFF, 0, 0, 10, 10),        # no such picture
        (0, 5, 5, 0, 10), (0, 5, 5, 10, 0),                   # empty
        (0, 170, 0, 7, 10), (0, 0, 140, 10, 5),               # one pixel over the right / the lower edge
        (0, 65530, 0, 20, 10), (0, 0, 65530, 10, 20),         # x + w = 65536 + 14: a 16-bit sum would wrap into the picture
        (1, 100, 100, 76, 44),                                # valid again, behind the invalid ones
    ]),
    "cif_wide_64x8": (CIF, 2, "random", (64, 8), [
        (1, 33, 7, 300, 200),                                 # 301 source columns from c0 = 32 on: two LDS chunks, x odd
        (0, 1, 0, 351, 288),
    ]),
    "qcif_identity": (QCIF, 1, "random", (176, 144), [
        (0, 0, 0, 176, 144),                                  # W' = w, H' = h
        (0, 17, 9, 50, 40),
    ]),
    "odd_width_33x7": (ODD, 2, "random", (33, 7), [
        (1, 5, 3, 170, 45),
        (0, 177, 49, 1, 1),
        (1, 0, 0, 178, 50),
        (1, 100, 10, 78, 40),                                 # ends at the buffer's last byte
    ]),
    "white_20x10": (QCIF, 1, "white", (20, 10), [
        (0, 0, 0, 176, 144), (0, 3, 3, 7, 5), (0, 175, 0, 1, 144),
    ]),
}
ALL_HAZARDS = {"one_pixel_source", "enlarging", "shrinking", "over_256_columns_odd_x", "last_byte_of_the_buffer", "identity",
               "one_column_last_segment", "one_row_last_band", "overlapping", "descending_pictures", "quotient_255", "byte_load_path",
               "invalid_reserved", "invalid_picture", "invalid_empty_w", "invalid_empty_h", "invalid_right_edge", "invalid_lower_edge",
               "invalid_x_plus_w_wraps_16_bits", "invalid_y_plus_h_wraps_16_bits", "valid_behind_invalid"}
# name -> (dtype, bgr, (scale, bias), base in elements, padded strides?)
PLACEMENTS = {
    "f32_padded": (tref.F32, False, tref.IMAGENET, 3, True),
    "f16_odd_base_odd_stride": (tref.F16, True, tref.EDGES, 1, True),
    "bf16_odd_base_odd_stride": (tref.BF16, False, tref.IMAGENET, 1, True),
    "bf16_contiguous": (tref.BF16, False, tref.IMAGENET, 0, False),
}
ALL_PLACEMENT_HAZARDS = {"16_bit_odd_base_odd_stride_h", "default_strides", "f32", "f16", "bf16"}


def pictures(name):
    """the table's full-size pictures: (h, w, 4) uint8, alpha 255"""
    (w, h), n, kind, _, _ = TABLES[name]
    if kind == "white":
        return [np.full((h, w, 4), 255, np.uint8) for _ in range(n)]
    rng = np.random.default_rng(w * 11 + h * 17 + n)
    out = [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for _ in range(n)]
    for p in out:
        p[:, :, 3] = 255
    return out


def placement(name, which, n_rois=None):
    """-> dict: dtype, bgr, scale, bias, base, the strides spelled out (stride_*), the strides as the caller passes them
    (arg_stride_*: 0 = default) and `elements`, the canvas's size: 9 elements behind the last tensor"""
    _, _, _, (ow, oh), rois = TABLES[name]
    n = len(rois) if n_rois is None else n_rois
    dtype, bgr, (scale, bias), base, padded = PLACEMENTS[which]
    if padded:
        stride_h = ow + 3 if (ow + 3) % 2 else ow + 4         # odd: the rows of a 16-bit tensor alternate between aligned and not
        stride_c = oh * stride_h + 5
        stride_n = 3 * stride_c + 7
        args = (stride_n, stride_c, stride_h)
    else:
        stride_h, stride_c, stride_n = ow, oh * ow, 3 * oh * ow
        args = (0, 0, 0)
    extent = (n - 1) * stride_n + 2 * stride_c + (oh - 1) * stride_h + ow if n else 0
    return dict(dtype=dtype, bgr=bgr, scale=scale, bias=bias, base=base, stride_n=stride_n, stride_c=stride_c, stride_h=stride_h,
                arg_stride_n=args[0], arg_stride_c=args[1], arg_stride_h=args[2], extent=extent, elements=base + extent + 9)


def placement_hazards(which):
    dtype, _, _, base, padded = PLACEMENTS[which]
    out = {{tref.F32: "f32", tref.F16: "f16", tref.BF16: "bf16"}[dtype]}
    if dtype != tref.F32 and base % 2 and padded:
        out.add("16_bit_odd_base_odd_stride_h")
    if not padded:
        out.add("default_strides")
    return out


def hazards(name):
    """what the table makes the kernel meet"""
    (w, h), n, kind, (ow, oh), rois = TABLES[name]
    out = set()
    if w % 4:
        out.add("byte_load_path")
    if ow % COLS_PER_SEGMENT == 1 and ow > COLS_PER_SEGMENT:
        out.add("one_column_last_segment")
    if oh % ROWS_PER_BAND == 1 and oh > ROWS_PER_BAND:
        out.add("one_row_last_band")
    ok = [ref.valid(r, n, w, h) for r in rois]
    seen_invalid = False
    for k, roi in enumerate(rois):
        p, x, y, rw, rh, reserved = ref.fields(roi)
        if not ok[k]:
            seen_invalid = True
            # each way alone: the other conditions hold
            others_fine = p < n and reserved == 0
            if reserved and p < n and 1 <= rw and 1 <= rh and x + rw <= w and y + rh <= h:
                out.add("invalid_reserved")
            if p >= n and not reserved:
                out.add("invalid_picture")
            if others_fine and rw == 0 and rh >= 1:
                out.add("invalid_empty_w")
            if others_fine and rh == 0 and rw >= 1:
                out.add("invalid_empty_h")
            if others_fine and rw >= 1 and rh >= 1 and y + rh <= h and x + rw > w:
                out.add("invalid_x_plus_w_wraps_16_bits" if (x + rw) % 65536 <= w and x + rw >= 65536 else "invalid_right_edge")
            if others_fine and rw >= 1 and rh >= 1 and x + rw <= w and y + rh > h:
                out.add("invalid_y_plus_h_wraps_16_bits" if (y + rh) % 65536 <= h and y + rh >= 65536 else "invalid_lower_edge")
            continue
        if seen_invalid:
            out.add("valid_behind_invalid")
        if rw == 1 and rh == 1:
            out.add("one_pixel_source")
        if rw < ow:
            out.add("enlarging")
        if rw > ow and rh > oh:
            out.add("shrinking")
        if (x, y, rw, rh) == (0, 0, w, h) and (ow, oh) == (w, h):
            out.add("identity")
        if p == n - 1 and x + rw == w and y + rh == h:
            out.add("last_byte_of_the_buffer")
        if kind == "white":
            out.add("quotient_255")
        for x0 in range(0, ow, COLS_PER_SEGMENT):
            x1 = min(x0 + COLS_PER_SEGMENT, ow) - 1
            first, last = x + x0 * rw // ow, x + ((x1 + 1) * rw - 1) // ow
            if last + 1 - (first & ~3) > CHUNK and x % 2 and (first & ~3) < x:
                out.add("over_256_columns_odd_x")
        for j in range(k):
            q, x2, y2, w2, h2, _ = ref.fields(rois[j])
            if ok[j] and q == p and x < x2 + w2 and x2 < x + rw and y < y2 + h2 and y2 < y + rh:
                out.add("overlapping")
            if ok[j] and q > p:
                out.add("descending_pictures")
    return out
