"""The reference of the motion regions (include/h263mi.h, MOTION REGIONS) in Python and numpy: the changed cells by the rule of the
change maps, the components by a breadth-first flood fill from every cell in raster order -- deliberately not the kernel's
union-find --, then boxes, stats, info, table and counts exactly as the contract words them.  Shared by the CPU checker's tests and
the GPU tests."""
from collections import deque

import numpy as np

INVALID_ROI = (0xFFFFFFFF, 0, 0, 0, 0, 1)
ZERO_STAT = (0, 0, 0)
NEIGHBOURS = {4: ((-1, 0), (0, -1), (0, 1), (1, 0)),
              8: ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))}


def changed_mask(grid, w, h, c, threshold):
    """(gh, gw) cell SADs -> bool: sad * c*c > threshold * pixels(cell), pixels(cell) = min(c, W - cx*c) * min(c, H - cy*c)"""
    gh, gw = grid.shape
    pix = np.minimum(c, h - np.arange(gh, dtype=np.int64) * c)[:, None] * np.minimum(c, w - np.arange(gw, dtype=np.int64) * c)[None, :]
    return grid.astype(np.int64) * (c * c) > np.int64(threshold) * pix           # (below 2^45)


def components(mask, connectivity):
    """-> [(label, [(cy, cx), ...])] in ascending label order; label = the smallest raster index of the component"""
    gh, gw = mask.shape
    seen = np.zeros_like(mask, dtype=bool)
    nb = NEIGHBOURS[connectivity]
    out = []
    for cy, cx in zip(*np.nonzero(mask)):                 # raster order: a component is met at its smallest index first
        cy, cx = int(cy), int(cx)
        if seen[cy, cx]:
            continue
        seen[cy, cx] = True
        cells, todo = [], deque([(cy, cx)])
        while todo:
            y, x = todo.popleft()
            cells.append((y, x))
            for dy, dx in nb:
                v, u = y + dy, x + dx
                if 0 <= v < gh and 0 <= u < gw and mask[v, u] and not seen[v, u]:
                    seen[v, u] = True
                    todo.append((v, u))
        out.append((cy * gw + cx, cells))
    return out


def box(cells, gw, gh, w, h, c, margin):
    """the cell bounding box, grown by margin cells and clipped to the grid, in pixels -> (x, y, w, h)"""
    cx0 = max(min(x for _, x in cells) - margin, 0)
    cy0 = max(min(y for y, _ in cells) - margin, 0)
    cx1 = min(max(x for _, x in cells) + margin, gw - 1)
    cy1 = min(max(y for y, _ in cells) + margin, gh - 1)
    x, y = cx0 * c, cy0 * c
    return x, y, min(w, (cx1 + 1) * c) - x, min(h, (cy1 + 1) * c) - y


def picture(grid, w, h, c, threshold, connectivity, margin, min_cells, max_per):
    """-> (components, kept, [(box, (sad, cells, label))] of the emitted components)"""
    gh, gw = grid.shape
    comps = components(changed_mask(grid, w, h, c, threshold), connectivity)
    kept = [(label, cells) for label, cells in comps if len(cells) >= min_cells]
    emitted = [(box(cells, gw, gh, w, h, c, margin), (sum(int(grid[y, x]) for y, x in cells), len(cells), label))
               for label, cells in kept[:max_per]]
    return len(comps), len(kept), emitted


def table(grids, w, h, c, threshold, connectivity, margin, min_cells, max_per, max_rois, summary_changed=None):
    """grids: (n, gh, gw); summary_changed: per picture the changed_cells of its summary, or None
    -> (rois: max_rois tuples (picture, x, y, w, h, reserved), stats: max_rois tuples (sad, cells, label),
        info: n tuples (components, kept, first, written), (count written, count wanted))"""
    rois, stats, info, total = [], [], [], 0
    for p, grid in enumerate(grids):
        if summary_changed is not None and summary_changed[p] == 0:
            info.append((0, 0, 0, 0))                     # not read at all
            continue
        ncomp, nkept, emitted = picture(grid, w, h, c, threshold, connectivity, margin, min_cells, max_per)
        first = min(total, max_rois)
        written = min(len(emitted), max_rois - first)
        info.append((ncomp, nkept, first, written))
        for b, s in emitted[:written]:
            rois.append((p,) + b + (0,))
            stats.append(s)
        total += len(emitted)
    count = len(rois)
    assert count == min(total, max_rois)
    rois += [INVALID_ROI] * (max_rois - count)
    stats += [ZERO_STAT] * (max_rois - count)
    return rois, stats, info, (count, total)
