"""numpy restatement of the resized RGBA output (include/h263mi.h: h263mi_rgba_resize) -- TEST INFRASTRUCTURE.

weights(w, ow): the ow x w matrix ox(X, i) = max(0, min((X+1)w, (i+1)W') - max(Xw, iW')) -- output column X covers [Xw, (X+1)w),
source column i covers [iW', (i+1)W'); every row sums to w.  The same with h, H' for rows.
resize: the full-size RGBA P -> (H', W', 4): (sum_j sum_i oy(Y,j) ox(X,i) P[j][i][c] + floor(wh/2)) // (wh), alpha 255.
extent: h263mi_rgba_resize_extent restated (None where the resize is refused).
Pinned by tests/golden/rgba_resize_known_answers.json (tests/test_rgba_resize.py).
"""
import numpy as np

import rgba_layout_ref


def weights(w, ow):
    X = np.arange(ow, dtype=np.int64)[:, None]
    i = np.arange(w, dtype=np.int64)[None, :]
    lo = np.maximum(X * w, i * ow)
    hi = np.minimum((X + 1) * w, (i + 1) * ow)
    return np.maximum(0, hi - lo)


def spans(w, ow):
    """the weights as (index, weight) pairs: (ow, K) arrays, output column X = sum_k weight[X, k] * column index[X, k]
    (the same numbers as weights(); unused slots have weight 0)"""
    X = np.arange(ow, dtype=np.int64)[:, None]
    first = X * w // ow
    k = np.arange(-(-w // ow) + 1, dtype=np.int64)[None, :]
    i = first + k
    wt = np.maximum(0, np.minimum((X + 1) * w, (i + 1) * ow) - np.maximum(X * w, i * ow))
    return np.minimum(i, w - 1), wt


def resize(rgba, w, h, ow, oh):
    """rgba: w*h*4 bytes (or an (h, w, 4) array) -> (H', W', 4) uint8"""
    p = np.asarray(rgba, np.uint8).reshape(h, w, 4)[:, :, :3].astype(np.int64)
    (iy, wy), (ix, wx) = spans(h, oh), spans(w, ow)
    t = np.zeros((oh, w, 3), np.int64)
    for k in range(iy.shape[1]):
        t += wy[:, k, None, None] * p[iy[:, k]]
    s = np.zeros((oh, ow, 3), np.int64)
    for k in range(ix.shape[1]):
        s += wx[None, :, k, None] * t[:, ix[:, k]]
    d = w * h
    out = np.full((oh, ow, 4), 255, np.uint8)
    out[:, :, :3] = (s + d // 2) // d
    return out


def extent(n, ow, oh, row_pitch=0, offsets=None, reserved=0):
    """bytes of h263mi_rgba_resize_extent, or None where it answers H263MI_ERR_INVALID_ARGUMENT"""
    if ow == 0 or oh == 0 or reserved:
        return None
    e = rgba_layout_ref.extent(n, ow, oh, 0, row_pitch, offsets)
    return None if e is None else e[2]


def routed_scale(w, h, ow, oh):
    """the scale_log2 of the layout that a resize is by definition, or None"""
    for f in range(3):
        m = (1 << f) - 1
        if not (w & m) and not (h & m) and ow == w >> f and oh == h >> f:
            return f
    return None
