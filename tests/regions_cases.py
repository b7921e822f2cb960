"""The cases of the motion regions (h263mi_regions_on), shared by the CPU checker's tests and the GPU tests.  The input is the cell
grid, so every case is synthetic: a boolean pattern becomes cell SADs (changed cells well above the threshold, the others at or below
what their pixels allow), a few cases set the SADs of edge cells by hand.  check_hazards() asserts, on the reference's side, that
each hazard the cases are there for occurs.

A grid of 32768 x 1 cells, which one might want at the cap, does not exist: a side has at most ceil(65535 / 8) = 8192 cells.  The cap
is met at 256 x 128 and at the widest and tallest grids there are, 8192 x 4 and 4 x 8192."""
import functools

import numpy as np

import regions_ref as ref

GARBAGE = 0xC3C3C3C3
THR = 100


class Case:
    def __init__(self, w, h, cl, grids, thr=THR, conn=8, margin=0, min_cells=1, max_per=16, max_rois=None, summary=None, stats=True):
        self.w, self.h, self.cl, self.c = w, h, cl, 1 << cl
        self.gw, self.gh = -(-w // self.c), -(-h // self.c)
        self.grids = np.ascontiguousarray(grids, dtype=np.uint32).reshape(-1, self.gh, self.gw)
        self.n = self.grids.shape[0]
        self.thr, self.conn, self.margin, self.min_cells, self.max_per = thr, conn, margin, min_cells, max_per
        self.max_rois = max_rois if max_rois is not None else max(1, min(65535, self.n * max_per))
        self.summary = summary                    # per picture the changed_cells of a summary, or None
        self.stats = stats
        assert self.gw * self.gh <= 32768

    def expected(self):
        return ref.table(self.grids, self.w, self.h, self.c, self.thr, self.conn, self.margin, self.min_cells, self.max_per,
                         self.max_rois, self.summary)

    def summaries(self):
        """the summary records handed to the call (sad and max_cell_sad are not looked at)"""
        return None if self.summary is None else [(0, int(v), 0) for v in self.summary]


def sads(mask, w, h, c, seed=0, thr=THR):
    """a pattern -> cell SADs: a changed cell well above the threshold, any other at most what keeps it unchanged"""
    mask = np.asarray(mask, dtype=bool)
    gh, gw = mask.shape
    rng = np.random.default_rng(seed)
    pix = np.minimum(c, h - np.arange(gh) * c)[:, None] * np.minimum(c, w - np.arange(gw) * c)[None, :]
    off = rng.integers(0, thr + 1, mask.shape) * pix // (c * c)
    on = thr + 1 + rng.integers(0, 1 << 20, mask.shape)
    return np.where(mask, on, off).astype(np.uint32)


def blobs(gh, gw, density, seed):
    return np.random.default_rng(seed).random((gh, gw)) < density


def serpentine(gh, gw):
    m = np.zeros((gh, gw), bool)
    m[0::2] = True
    for k, y in enumerate(range(1, gh, 2)):
        if y + 1 < gh:
            m[y, gw - 1 if k % 2 == 0 else 0] = True
    return m


def spiral(gh, gw):
    m = np.zeros((gh, gw), bool)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    inside = lambda v, u: 0 <= v < gh and 0 <= u < gw
    while True:
        for _ in range(2):
            v, u, v2, u2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if inside(v, u) and not m[v, u] and (not inside(v2, u2) or not m[v2, u2]):
                y, x = v, u
                m[y, x] = True
                break
            dy, dx = dx, -dy                      # turn right
        else:
            return m


def comb(gh, gw):
    m = np.zeros((gh, gw), bool)
    m[:, 0::2] = True
    m[gh - 1] = True
    return m


def two_us(gh, gw):
    """two nested U shapes, each joined only in its last row, and both joined by the very last row"""
    m = np.zeros((gh, gw), bool)
    m[:, 0] = m[:, gw - 1] = True
    m[gh - 1] = True
    m[:gh - 2, 2] = m[:gh - 2, gw - 3] = True
    m[gh - 3, 2:gw - 2] = True
    m[gh - 2, gw // 2] = True
    return m


def pattern(text):
    return np.array([[ch == "#" for ch in row] for row in text.split()], bool)


def of_mask(mask, cl=3, w=None, h=None, seed=0, **kw):
    mask = np.asarray(mask, bool)
    masks = mask if mask.ndim == 3 else mask[None]
    c = 1 << cl
    w = masks.shape[2] * c if w is None else w
    h = masks.shape[1] * c if h is None else h
    return Case(w, h, cl, np.stack([sads(m, w, h, c, seed + k) for k, m in enumerate(masks)]), **kw)


def edge_cells(cl):
    """W and H no multiples of c: the right column is q = c/2 + 1 pixels wide, the bottom row 3 pixels high.  By hand: edge cells at
    the threshold's exact scale (equal: unchanged, one more: changed), edge cells whose raw SAD is at or below the threshold and
    that are changed all the same, and full cells with the very same SADs that are not"""
    c = 1 << cl
    q = c // 2 + 1
    w, h = 3 * c + q, 2 * c + 3
    thr = 4 * c * c                                # thr * pixels is a multiple of c*c for every cell
    g = np.zeros((3, 4), np.uint32)
    right, bottom, corner = thr * q * c // (c * c), thr * 3 * c // (c * c), thr * 3 * q // (c * c)
    g[0, 3] = right                                # exactly the scaled threshold: unchanged
    g[1, 3] = right + 1                            # changed, raw SAD far below thr
    g[2, 0] = bottom + 1                           # changed
    g[2, 1] = bottom                               # unchanged
    g[2, 3] = corner + 1                           # changed
    g[0, 0] = thr                                  # a full cell at the threshold: unchanged
    g[0, 1] = right + 1                            # a full cell with the SAD that changes an edge cell: unchanged
    g[1, 1] = thr + 1                              # a full cell: changed
    return Case(w, h, cl, g[None], thr=thr, conn=4, max_per=8)


def borders(margin, cl=4):
    """a blob in every corner, one on every side and one in the middle; partial cells on the right and at the bottom"""
    c = 1 << cl
    gh, gw = 21, 25
    m = np.zeros((gh, gw), bool)
    for y in (0, gh // 2, gh - 1):
        for x in (0, gw // 2, gw - 1):
            m[y, x] = True
    m[gh // 2, gw // 2 + 1] = True
    return of_mask(m, cl, w=gw * c - 5, h=gh * c - 9, margin=margin, max_per=16, seed=margin)


def many_pictures(n):
    gh, gw = 6, 9
    masks = np.zeros((n, gh, gw), bool)
    for p in range(n):
        if p % 3 != 1:                             # every third picture is empty
            masks[p] = blobs(gh, gw, 0.3, 100 + p)
    return of_mask(masks, 3, w=gw * 8 - 3, h=gh * 8 - 1, conn=4, max_per=3, max_rois=max(1, 2 * n), seed=n)


def skip_case():
    gh, gw = 5, 7
    masks = np.stack([blobs(gh, gw, 0.4, 1), np.zeros((gh, gw), bool), blobs(gh, gw, 0.4, 2), np.zeros((gh, gw), bool)])
    k = of_mask(masks, 4, conn=8, max_per=4)
    k.grids[1] = GARBAGE                           # never written: a stream without a picture
    k.grids[3] = GARBAGE
    k.summary = [int(masks[0].sum()), 0, int(masks[2].sum()), 0]
    return k


def skip_by_the_summary_alone():
    """the rule is the summary's zero, whatever the grid holds: a picture full of changed cells is skipped too"""
    k = of_mask(np.ones((2, 3, 3), bool), 3)
    k.summary = [0, 9]
    return k


DIAG = pattern("#.... .#... ..#.. ...#. ....#")
ANTI = pattern("....# ...#. ..#.. .#... #....")
THREE = pattern("##..#..### ##..#..... ....#..#.. .......#..")      # four components: 4, 3, 3 and 2 cells, labels 0, 4, 7 and 27

CASES = {
    # ---- grid shapes
    "grid_1x1_on": lambda: of_mask(np.ones((1, 1), bool), 3, w=1, h=1),
    "grid_1x1_off": lambda: of_mask(np.zeros((1, 1), bool), 6),
    "grid_row_70": lambda: of_mask(blobs(1, 70, 0.6, 3), 3, w=70 * 8 - 7),
    "grid_col_70": lambda: of_mask(blobs(70, 1, 0.6, 4), 3, h=70 * 8 - 1),
    "grid_63_c4": lambda: of_mask(blobs(7, 63, 0.45, 5), 3, conn=4, max_per=256),
    "grid_63_c8": lambda: of_mask(blobs(7, 63, 0.45, 5), 3, conn=8, max_per=256),
    "grid_64_c4": lambda: of_mask(blobs(7, 64, 0.5, 6), 3, conn=4, max_per=256),
    "grid_64_c8": lambda: of_mask(blobs(7, 64, 0.4, 6), 3, conn=8, max_per=256),
    "grid_65_c4": lambda: of_mask(blobs(7, 65, 0.55, 7), 3, conn=4, max_per=256),
    "grid_65_c8": lambda: of_mask(blobs(7, 65, 0.35, 7), 3, conn=8, max_per=256),
    "grid_2_rows": lambda: of_mask(blobs(2, 130, 0.5, 8), 3, conn=8, max_per=64),
    "grid_full_rows": lambda: of_mask(np.ones((3, 200), bool), 3, conn=4),
    "cap_256x128_c4": lambda: of_mask(blobs(128, 256, 0.55, 9), 3, conn=4, max_per=256, min_cells=3),
    "cap_256x128_c8": lambda: of_mask(blobs(128, 256, 0.4, 10), 3, conn=8, max_per=256, min_cells=3),
    "cap_8192x4": lambda: of_mask(blobs(4, 8192, 0.6, 11), 3, w=65535, conn=8, max_per=256, min_cells=40),
    "cap_4x8192": lambda: of_mask(blobs(8192, 4, 0.6, 12), 3, h=65535, conn=4, max_per=256, min_cells=40),
    "cap_8192x4_one_run": lambda: of_mask(np.ones((4, 8192), bool), 3, w=65535, conn=4),
    "cap_4x8192_columns": lambda: of_mask(np.tile(np.array([True, False, True, False]), (8192, 1)), 3, h=65535, conn=4),
    # ---- edge cells
    "edge_cells_c8": lambda: edge_cells(3),
    "edge_cells_c16": lambda: edge_cells(4),
    "edge_cells_c32": lambda: edge_cells(5),
    "edge_cells_c64": lambda: edge_cells(6),
    # ---- connectivity
    "diagonal_c8": lambda: of_mask(DIAG, 4, conn=8),
    "diagonal_c4": lambda: of_mask(DIAG, 4, conn=4),
    "down_left_diagonal_c8": lambda: of_mask(ANTI, 4, conn=8),
    "down_left_diagonal_c4": lambda: of_mask(ANTI, 4, conn=4),
    "down_left_corner_of_runs_c8": lambda: of_mask(pattern("...### ###... ...### ###..."), 5, conn=8),
    "checkerboard_cap_c8": lambda: of_mask(np.indices((128, 256)).sum(0) % 2 == 0, 3, conn=8, max_per=4),
    "checkerboard_cap_c4": lambda: of_mask(np.indices((128, 256)).sum(0) % 2 == 0, 3, conn=4, max_per=256, max_rois=300),
    # ---- long paths
    "serpentine_cap": lambda: of_mask(serpentine(128, 256), 3, conn=4, margin=1),
    "serpentine_cap_c8": lambda: of_mask(serpentine(128, 256), 3, conn=8),
    "serpentine_tall": lambda: of_mask(serpentine(128, 256).T, 3, conn=4),
    "spiral_cap": lambda: of_mask(spiral(128, 256), 3, conn=4),
    "spiral_135x240": lambda: of_mask(spiral(135, 240), 3, w=1920, h=1080, conn=4),
    "comb": lambda: of_mask(comb(60, 131), 3, conn=4),
    "comb_upside_down": lambda: of_mask(comb(60, 131)[::-1], 3, conn=4),
    "two_us": lambda: of_mask(two_us(40, 71), 3, conn=4),
    "two_us_c8": lambda: of_mask(two_us(40, 71), 3, conn=8),
    # ---- filters
    "min_cells_exact": lambda: of_mask(THREE, 3, conn=4, min_cells=3),
    "min_cells_one_above": lambda: of_mask(THREE, 3, conn=4, min_cells=4),
    "min_cells_huge": lambda: of_mask(THREE, 3, conn=4, min_cells=0xFFFFFFFF),
    "max_per_below_kept": lambda: of_mask(THREE, 3, conn=4, max_per=3),
    "max_per_at_kept": lambda: of_mask(THREE, 3, conn=4, max_per=4),
    "max_per_above_kept": lambda: of_mask(THREE, 3, conn=4, max_per=5),
    "max_per_1": lambda: of_mask(np.stack([THREE, THREE[::-1]]), 3, conn=4, max_per=1),
    "table_full_mid_picture": lambda: of_mask(np.stack([THREE, THREE, THREE]), 3, conn=4, max_per=4, max_rois=6),
    "table_full_at_a_picture": lambda: of_mask(np.stack([THREE, THREE, THREE]), 3, conn=4, max_per=4, max_rois=8),
    "max_rois_1": lambda: of_mask(np.stack([np.zeros_like(THREE), THREE, THREE]), 3, conn=4, max_per=4, max_rois=1),
    "max_rois_65535": lambda: of_mask(THREE, 3, conn=4, max_per=4, max_rois=65535),
    "without_stats": lambda: of_mask(np.stack([THREE, THREE]), 3, conn=4, max_per=4, max_rois=11, stats=False),
    # ---- boxes
    "margin_0_borders": lambda: borders(0),
    "margin_1_borders": lambda: borders(1),
    "margin_8_borders": lambda: borders(8),
    "margin_8_small_grid": lambda: of_mask(pattern("... .#. ..."), 6, w=3 * 64 - 63, h=3 * 64 - 1, margin=8),
    "box_partial_right_bottom": lambda: of_mask(pattern(".... ..## ..##"), 4, w=4 * 16 - 7, h=3 * 16 - 11, conn=4),
    # ---- skip
    "skip_garbage": skip_case,
    "skip_by_summary_alone": skip_by_the_summary_alone,
    "summary_without_zeros": lambda: of_mask(np.stack([THREE, THREE]), 3, conn=4, summary=[3, 1]),
    # ---- pictures
    "pictures_1": lambda: many_pictures(1),
    "pictures_2": lambda: many_pictures(2),
    "pictures_130": lambda: many_pictures(130),
}

# what each mutant of mutants.h must fail
MUTANT_CASES = {
    "H263MI_MUTATE_REGIONS_DIAGONAL": ["down_left_diagonal_c8", "down_left_corner_of_runs_c8", "checkerboard_cap_c8"],
    "H263MI_MUTATE_REGIONS_BOX_CLIP": ["box_partial_right_bottom", "margin_8_small_grid", "margin_1_borders"],
}


@functools.lru_cache(maxsize=None)
def build(name):
    """the case and its expected results, computed once and shared: treat both as read-only"""
    k = CASES[name]()
    k.want = k.expected()
    return k


def check_hazards():
    info = lambda name: build(name).want[2]
    one = lambda name: info(name)[0][0]
    # the grid shapes and the cap
    assert (build("grid_1x1_on").gw, build("grid_1x1_on").gh) == (1, 1) and one("grid_1x1_on") == 1 and one("grid_1x1_off") == 0
    assert build("grid_row_70").gh == 1 and build("grid_col_70").gw == 1 and one("grid_row_70") > 3 and one("grid_col_70") > 3
    assert [build("grid_%d_c4" % g).gw for g in (63, 64, 65)] == [63, 64, 65] and build("grid_2_rows").gh == 2
    for name in ("cap_256x128_c4", "cap_8192x4", "cap_4x8192", "checkerboard_cap_c4", "serpentine_cap", "spiral_cap"):
        assert build(name).gw * build(name).gh == 32768, name
    assert build("spiral_135x240").gw * build("spiral_135x240").gh == 32400
    assert one("cap_8192x4_one_run") == 1 and build("cap_8192x4_one_run").want[1][0][1] == 32768
    assert one("cap_4x8192_columns") == 2 and build("cap_4x8192_columns").want[1][0][1] == 8192
    # edge cells: changed with a raw SAD below the threshold, and a full cell with the same SAD that is not
    for cl in (3, 4, 5, 6):
        k = build("edge_cells_c%d" % (1 << cl))
        assert k.w % k.c and k.h % k.c
        mask = ref.changed_mask(k.grids[0], k.w, k.h, k.c, k.thr)
        assert mask.tolist() == [[False, False, False, False], [False, True, False, True], [True, False, False, True]]
        assert k.grids[0][1, 3] <= k.thr and k.grids[0][0, 1] == k.grids[0][1, 3] and k.grids[0][0, 3] + 1 == k.grids[0][1, 3]
    # connectivity
    assert one("diagonal_c8") == 1 and one("diagonal_c4") == 5 and one("down_left_diagonal_c8") == 1 and one("down_left_diagonal_c4") == 5
    assert one("down_left_corner_of_runs_c8") == 1
    assert one("checkerboard_cap_c8") == 1 and one("checkerboard_cap_c4") == 16384
    assert build("checkerboard_cap_c4").want[3] == (256, 256)
    # long paths: one component each, thousands of cells
    for name, conn_cells in (("serpentine_cap", 64 * 256 + 63), ("serpentine_cap_c8", 64 * 256 + 63), ("serpentine_tall", 64 * 256 + 63),
                             ("spiral_cap", None), ("spiral_135x240", None), ("comb", None), ("comb_upside_down", None), ("two_us", None)):
        k = build(name)
        assert one(name) == 1, name
        cells = k.want[1][0][1]
        assert cells == int(ref.changed_mask(k.grids[0], k.w, k.h, k.c, k.thr).sum()) and cells > 150
        assert conn_cells is None or cells == conn_cells
    assert build("spiral_cap").want[1][0][1] > 16000 and build("comb").want[1][0][1] > 4000
    # filters
    sizes = sorted(s[1] for s in build("max_per_above_kept").want[1][:4])
    assert sizes == [2, 3, 3, 4]
    assert info("min_cells_exact")[0][:2] == (4, 3) and info("min_cells_one_above")[0][:2] == (4, 1) and info("min_cells_huge")[0][:2] == (4, 0)
    assert [info(n)[0][3] for n in ("max_per_below_kept", "max_per_at_kept", "max_per_above_kept")] == [3, 4, 4]
    assert [i[2:] for i in info("table_full_mid_picture")] == [(0, 4), (4, 2), (6, 0)] and build("table_full_mid_picture").want[3] == (6, 12)
    assert [i[2:] for i in info("table_full_at_a_picture")] == [(0, 4), (4, 4), (8, 0)]
    assert [i[2:] for i in info("max_rois_1")] == [(0, 0), (0, 1), (1, 0)] and build("max_rois_1").want[3] == (1, 8)
    # boxes: every border is met by a margin, and the partial cells by a box
    for margin in (0, 1, 8):
        k = build("margin_%d_borders" % margin)
        boxes = [r[1:5] for r in k.want[0][:k.want[3][0]]]
        assert len(boxes) == 9
        assert any(x == 0 for x, y, w, h in boxes) and any(y == 0 for x, y, w, h in boxes)
        assert any(x + w == k.w for x, y, w, h in boxes) and any(y + h == k.h for x, y, w, h in boxes)
        assert all(x + w <= k.w and y + h <= k.h and w >= 1 and h >= 1 for x, y, w, h in boxes)
    k = build("box_partial_right_bottom")
    assert k.want[0][0][1:5] == (32, 16, k.w - 32, k.h - 16) and k.w % 16 and k.h % 16
    # skip
    k = build("skip_garbage")
    assert k.want[2][1] == k.want[2][3] == (0, 0, 0, 0) and (k.grids[1] == GARBAGE).all() and k.want[2][2][0] > 0
    assert build("skip_by_summary_alone").want[2] == [(0, 0, 0, 0), (1, 1, 0, 1)]
    # pictures
    assert [build("pictures_%d" % n).n for n in (1, 2, 130)] == [1, 2, 130]
    assert sum(1 for i in info("pictures_130") if i[0] == 0) >= 43 and info("pictures_130")[129][2] > 64


ROI = np.dtype([("picture", np.uint32), ("x", np.uint16), ("y", np.uint16), ("w", np.uint16), ("h", np.uint16), ("reserved", np.uint32)])
STAT = np.dtype([("sad", np.uint64), ("cells", np.uint32), ("label", np.uint32)])
INFO = np.dtype([("components", np.uint32), ("kept", np.uint32), ("first", np.uint32), ("written", np.uint32)])
SUMMARY = np.dtype([("sad", np.uint64), ("changed_cells", np.uint32), ("max_cell_sad", np.uint32)])


def compare(k, rois, stats, info, count):
    """None, or what differs from the reference.  rois (ROI, max_rois), stats (STAT, max_rois; None: not asked for), info (INFO, n)
    and count (two uint32) are the outputs' bytes as they are after the launch: every entry of the table is compared, the invalid tail
    too"""
    want_rois, want_stats, want_info, want_count = k.want
    if tuple(int(v) for v in count) != want_count:
        return "counts %r, want %r" % (tuple(int(v) for v in count), want_count)
    if [tuple(int(v) for v in i) for i in info] != want_info:
        bad = [p for p in range(k.n) if tuple(int(v) for v in info[p]) != want_info[p]][0]
        return "info of picture %d: %r, want %r" % (bad, info[bad], want_info[bad])
    want = np.array(want_rois, dtype=ROI)
    if rois.tobytes() != want.tobytes():
        bad = [j for j in range(k.max_rois) if rois[j] != want[j]][0]
        return "entry %d: %r, want %r" % (bad, rois[bad], want[bad])
    if stats is not None:
        want = np.array(want_stats, dtype=STAT)
        if stats.tobytes() != want.tobytes():
            bad = [j for j in range(k.max_rois) if stats[j] != want[j]][0]
            return "stat %d: %r, want %r" % (bad, stats[bad], want[bad])
    return None
