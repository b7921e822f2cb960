"""Restatement of the ROI crop-and-resize (include/h263mi.h: h263mi_roi, h263mi_roi_tensor_on) -- TEST INFRASTRUCTURE.

It adds no arithmetic of its own: a valid ROI's tensor is framing_ref.rgba of the WINDOW (x, y, w, h) -> (0, 0, W', H') of its
picture, then tensor_out_ref.planes.

valid(roi, n_pictures, width, height): the per-ROI rule, in Python integers (nothing wraps).
crop(pictures, roi, ow, oh): the (H', W', 4) RGBA of a valid ROI; computed once per (pictures, roi, size) by the callers' caches.
expected(canvas, crops, rois, ...): the element canvas after the call and the status words; an invalid ROI leaves its elements
    as they were.
A ROI is (picture, x, y, w, h) or (picture, x, y, w, h, reserved).
"""
import numpy as np

import framing_ref
import tensor_out_ref


def fields(roi):
    picture, x, y, w, h = roi[:5]
    return picture, x, y, w, h, (roi[5] if len(roi) > 5 else 0)


def valid(roi, n_pictures, width, height):
    picture, x, y, w, h, reserved = fields(roi)
    return reserved == 0 and picture < n_pictures and w >= 1 and h >= 1 and x + w <= width and y + h <= height


def crop(pictures, roi, ow, oh):
    """pictures: a list of (h, w, 4) uint8 arrays -> (H', W', 4) uint8 of a valid ROI"""
    picture, x, y, w, h, _ = fields(roi)
    return framing_ref.rgba(pictures[picture], ow, oh, ((x, y, w, h), (0, 0, ow, oh)))


def expected(canvas, crops, rois, n_pictures, width, height, dtype, scale, bias, bgr, base, stride_n, stride_c, stride_h):
    """canvas: 1-D array of element bit patterns; crops[k]: crop() of ROI k (looked at for valid ROIs only); the strides and
    `base` in elements, spelled out -> (the canvas after the call, the status words)"""
    want = canvas.copy()
    status = np.zeros(len(rois), np.uint32)
    for k, roi in enumerate(rois):
        if not valid(roi, n_pictures, width, height):
            status[k] = 1
            continue
        pl = tensor_out_ref.planes(crops[k], dtype, scale, bias, bgr)
        tensor_out_ref.place(want, pl, base + k * stride_n, stride_c, stride_h)
    return want, status
