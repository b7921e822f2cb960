"""The numpy reference of the change maps (include/h263mi.h, CHANGE MAPS): cell SADs by np.add.reduceat over |cur - prev|, then the
comparison, the summaries and the selection in Python integers.  Shared by the CPU checker's tests and the GPU tests."""
import numpy as np


def cells(cur, prev, c):
    """(n, H, W) uint8 planes -> (n, gh, gw) int64 cell SADs; edge cells hold what the picture holds of them"""
    d = np.abs(cur.astype(np.int64) - prev.astype(np.int64))
    return np.add.reduceat(np.add.reduceat(d, np.arange(0, d.shape[1], c), axis=1), np.arange(0, d.shape[2], c), axis=2)


def pixels(w, h, c, cy, cx):
    return min(c, w - cx * c) * min(c, h - cy * c)


def changed(sad, c, threshold, npix):
    return int(sad) * c * c > threshold * npix


def summaries(grid, w, h, c, threshold, valid=None):
    """-> [(sad, changed_cells, max_cell_sad)] per picture; an invalid picture's is all zero"""
    out = []
    for p, g in enumerate(grid):
        if valid is not None and not valid[p]:
            out.append((0, 0, 0))
            continue
        n = sum(changed(g[cy, cx], c, threshold, pixels(w, h, c, cy, cx)) for cy in range(g.shape[0]) for cx in range(g.shape[1]))
        out.append((int(g.sum()), n, int(g.max())))
    return out


def select(summ, min_changed, valid=None):
    """the indices of the valid pictures with changed_cells >= min_changed, ascending"""
    return [p for p, s in enumerate(summ) if (valid is None or valid[p]) and s[1] >= min_changed]
