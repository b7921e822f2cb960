"""Designed inputs for the deblocking post-filter (deblock/src/deblock.rs), and the classifier that says what they reach.

INPUTS ONLY, in the manner of mc_cases.py: expected bytes always come from the C oracle (oracle/h263_oracle.c), cross-checked
by the numpy restatement (oracle/np_restatement.py: deblock_trace).  The classifier works from the planes the oracle decodes
and from that restatement's per-quartet trace, never from GPU output.

Every filtered quartet A, B | C, D gets
  an ARITHMETIC CLASS (classify): division semantics (the reference's SIMD lanes shift = floor, its scalar tails divide =
      truncation), sign of d, ramp region (d = 0; 0 < |d| <= S; S < |d| < 2S; |d| >= 2S), d2 clip ((A - D) / 4 = 0; inside
      +-|d1 / 2|; clipped), rounding-sensitive limit (floor, d1 negative and odd, the clip active: the quartets on which
      |d1 / 2| rounded toward zero changes A and D), division-sensitive numerator (A - 4B + 4C - D < 0 and no multiple of 8;
      A - D < 0 and no multiple of 4), output saturation (B + d1 > 255, B + d1 < 0, C - d1 > 255, C - d1 < 0)
  a PLACEMENT (Placement): plane, direction (DIR_H: a horizontal block edge, A..D are four rows; DIR_V: a vertical one), packed
      half (even / odd column of a horizontal edge, even / odd row of a vertical one: the two 16-bit halves of
      deblock_quartet_pk), and the kinds of the post tile that filters it, by the kernel's own rules restated here
      (post_tile_columns, post_tile_is_interior_geom of csrc/post_kernel.inl): TILE_KINDS.

Table (a): ARITHMETIC, through the standalone deblock() of one plane (luma, the general form of the kernel).  The lattice of
  tests/sim/sim.cpp: sim_quartet_sweep -- every (A - D, C - B) in [-255, 255]^2, each difference at both ends of the byte
  range -- at one strength, every lattice point in each of floor / truncation x horizontal / vertical edge x low / high half.
  A plane 8 wide has no vertical edge (deblock.rs:228) and shifts in every column, one 7 wide divides in every column; the
  transposed planes (8 and 7 rows: no horizontal edge, deblock.rs:140) do the same for the vertical edges.  The arithmetic
  class space is not written down anywhere: it is what classify() makes of the lattice (class_space).

Table (b): PLACEMENT, through the frame store.  Planes enter a batch or a state by decoding only, so the inputs are records:
  seeded intra pictures whose macroblocks take one of THEMES -- levels of (Y, Cb, Cr) chosen so that samples near both ends of
  the byte range still show in an unclamped RGBA channel -- under a texture of a few small coefficients.  SIZES_B are the
  smallest pictures with every tile kind between them; one batch per size, its streams at the strengths 0..12 (twice).
  CONDITION (missing_b): for every tile kind x plane x direction x half, counted quartets show both signs of d, each
  non-zero ramp region, a clipped d2, a saturated output, and a rounding-sensitive limit (at floor positions) or a
  division-sensitive numerator (truncation kinds).  For outputs that are RGBA only a quartet counts only if each of its four
  samples drives an unclamped channel of the oracle's RGBA (so that +-1 in the sample shows); for plane outputs all count.
  Every picture goes through every output path, so the condition holds per path as it holds per way of counting.
  EXCLUSIONS, each a matter of geometry and asserted EMPTY by the classifier (geometry_exclusions):
    wrap x DIR_V         the columns that ride in the last tile take part in no vertical-edge quartet (the first is 6..9)
    left x DIR_V         tile column 0 holds picture columns 0..3 only: likewise
    trunc_cols x DIR_V   truncation columns are a property of horizontal-edge quartets (deblock.rs:164-177)
    trunc_rows x DIR_H   truncation rows are a property of vertical-edge quartets (deblock.rs:278-297)
    interior x trunc_*   an interior tile lies inside the region of the reference's SIMD lanes altogether
"""
import numpy as np

from oracle import np_restatement as npr
from oracle.oracle import MB_RECORD_DTYPE

DIR_H, DIR_V = npr.DIR_H, npr.DIR_V
DIR_NAMES = ("horizontal edge", "vertical edge")
PLANE_NAMES = ("Y", "Cb", "Cr")

# ---------------------------------------------------------------------------------------------------------------
# the arithmetic class of a quartet
# ---------------------------------------------------------------------------------------------------------------
CLASS_DTYPE = np.dtype([("floor", "?"), ("sign", "i1"), ("ramp", "u1"), ("d2clip", "u1"), ("roundsens", "?"),
                        ("divsens", "u1"), ("sat", "u1")])
SAT_NAMES = {1: "B+d1>255", 2: "B+d1<0", 4: "C-d1>255", 8: "C-d1<0"}


def classify(abcd, floor, strength):
    """CLASS_DTYPE per quartet: abcd uint8[n, 4] as the pass reads them, floor bool[n], one strength"""
    A, B, C, D = (abcd[:, k].astype(np.int64) for k in range(4))
    floor = np.asarray(floor, bool)
    S = int(strength)
    x, ad = A - 4 * B + 4 * C - D, A - D
    d = npr._div_pow2(x, 3, floor)
    m = np.abs(d)
    mag = np.maximum(m - np.maximum(2 * (m - S), 0), 0)
    d1 = np.sign(d) * mag
    lim = np.abs(npr._div_pow2(d1, 1, floor))
    q = npr._div_pow2(ad, 2, floor)
    out = np.zeros(len(abcd), CLASS_DTYPE)
    out["floor"] = floor
    out["sign"] = np.sign(d)
    out["ramp"] = np.where(m == 0, 0, np.where(m <= S, 1, np.where(m < 2 * S, 2, 3)))
    out["d2clip"] = np.where(q == 0, 0, np.where(np.abs(q) <= lim, 1, 2))
    out["roundsens"] = floor & (d1 < 0) & (mag % 2 == 1) & (np.abs(q) >= lim)
    out["divsens"] = ((x < 0) & (x % 8 != 0)) * 1 + ((ad < 0) & (ad % 4 != 0)) * 2
    out["sat"] = (B + d1 > 255) * 1 + (B + d1 < 0) * 2 + (C - d1 > 255) * 4 + (C - d1 < 0) * 8
    return out


def class_key(c):
    """one integer per class"""
    return (c["floor"].astype(np.int64) | ((c["sign"].astype(np.int64) + 1) << 1) | (c["ramp"].astype(np.int64) << 3) |
            (c["d2clip"].astype(np.int64) << 5) | (c["roundsens"].astype(np.int64) << 7) | (c["divsens"].astype(np.int64) << 8) |
            (c["sat"].astype(np.int64) << 10))


def describe_class(c):
    sat = "+".join(n for b, n in SAT_NAMES.items() if int(c["sat"]) & b) or "none"
    return ("%s, d %s, ramp region %d, d2 %s%s%s, saturation %s"
            % ("floor" if c["floor"] else "truncation", "-0+"[int(c["sign"]) + 1], int(c["ramp"]),
               ("zero", "inside", "clipped")[int(c["d2clip"])], ", rounding-sensitive" if c["roundsens"] else "",
               ", division-sensitive(%d)" % int(c["divsens"]) if c["divsens"] else "", sat))


# ---------------------------------------------------------------------------------------------------------------
# table (a)
# ---------------------------------------------------------------------------------------------------------------
_LATTICE = None


def lattice():
    """uint8[N, 4] = A, B, C, D of sim_quartet_sweep's quartets, in its order (x, end of x, y, end of y)"""
    global _LATTICE
    if _LATTICE is None:
        v = np.repeat(np.arange(-255, 256), 2)
        end = np.tile(np.arange(2), 511)
        hi = np.maximum(v, 0) + end * (255 - np.abs(v))          # the larger sample of the pair
        lo = hi - v
        n = v.size
        q = np.empty((n, n, 4), np.uint8)
        q[:, :, 0], q[:, :, 3] = hi[:, None], lo[:, None]        # A - D = x
        q[:, :, 2], q[:, :, 1] = hi[None, :], lo[None, :]        # C - B = y
        _LATTICE = q.reshape(-1, 4)
    return _LATTICE


def quartet_keys(abcd):
    a = np.asarray(abcd, np.uint32)
    return (a[:, 0] << 24) | (a[:, 1] << 16) | (a[:, 2] << 8) | a[:, 3]


_LATTICE_KEYS = None


def lattice_keys():
    """sorted, unique (the two ends of a difference of +-255 are the same quartet)"""
    global _LATTICE_KEYS
    if _LATTICE_KEYS is None:
        _LATTICE_KEYS = np.unique(quartet_keys(lattice()))
    return _LATTICE_KEYS


A_EDGES = 8191          # block edges of a table plane: 8 * 8191 + 2 = 65 530 rows (columns), the most a picture may have
A_CONFIGS = [(DIR_H, True), (DIR_H, False), (DIR_V, True), (DIR_V, False)]
FILL = 128


def table_a(direction, floor):
    """the planes of one configuration: dict(name, w, h, plane uint8[h, w], dir, floor).  The same planes serve every
    strength (the lattice does not depend on it).  A horizontal-edge plane is 8 (floor) or 7 (truncation) columns wide:
    edge e has its A..D rows at 8e + 6 .. 8e + 9, its even columns hold one run through the lattice, its odd columns
    another (half a lattice ahead), so that each half of the packed quartet sees every point.  A vertical-edge plane is
    the transpose."""
    L = lattice()
    N = len(L)
    width = 8 if floor else 7
    n_even, n_odd = (width + 1) // 2, width // 2
    edges = -(-N // n_odd)
    n_planes = -(-edges // A_EDGES)
    T = n_planes * A_EDGES
    idx = np.empty((T, width), np.int64)
    idx[:, 0::2] = (np.arange(T * n_even) % N).reshape(T, n_even)
    idx[:, 1::2] = ((np.arange(T * n_odd) + N // 2) % N).reshape(T, n_odd)
    rows = L[idx]                                                        # [edge, column, sample]
    for k in range(n_planes):
        p = np.full((A_EDGES + 1, 8, width), FILL, np.uint8)             # [block row, row of the block, column]
        p[:-1, 6:8] = rows[k * A_EDGES:(k + 1) * A_EDGES, :, 0:2].transpose(0, 2, 1)
        p[1:, 0:2] = rows[k * A_EDGES:(k + 1) * A_EDGES, :, 2:4].transpose(0, 2, 1)
        p = p.reshape(-1, width)[:8 * A_EDGES + 2]
        if direction == DIR_V:
            p = np.ascontiguousarray(p.T)
        yield dict(name="a-%s-%s-%02d" % ("hv"[direction], "floor" if floor else "trunc", k), w=p.shape[1], h=p.shape[0],
                   plane=p, dir=direction, floor=floor)


class CoverageA:
    """which lattice points and which classes the traces of table (a) hold, per (floor, direction, half)"""

    def __init__(self, strength):
        self.strength = strength
        self.seen = {}
        self.classes = {}

    def add(self, trace):
        cls = class_key(classify(trace["abcd"], trace["floor"], self.strength))
        keys = quartet_keys(trace["abcd"])
        half = np.where(trace["dir"] == DIR_H, trace["x"] & 1, trace["y"] & 1)
        for fl in (True, False):
            for direction in (DIR_H, DIR_V):
                for hf in (0, 1):
                    m = (trace["floor"] == fl) & (trace["dir"] == direction) & (half == hf)
                    if not m.any():
                        continue
                    k = (fl, direction, hf)
                    present = np.zeros(len(lattice_keys()), bool)
                    pos = np.searchsorted(lattice_keys(), keys[m])
                    pos[pos >= len(lattice_keys())] = 0
                    present[pos[lattice_keys()[pos] == keys[m]]] = True
                    self.seen[k] = self.seen.get(k, False) | present
                    self.classes.setdefault(k, {})
                    for c, n in zip(*np.unique(cls[m], return_counts=True)):
                        self.classes[k][int(c)] = self.classes[k].get(int(c), 0) + int(n)

    def missing(self, configs=A_CONFIGS):
        """(floor, direction, half, what) of everything the configurations should have shown and did not"""
        out = []
        for fl, direction in [(f, d) for d, f in configs]:
            space = class_space(self.strength, fl)
            for hf in (0, 1):
                k = (fl, direction, hf)
                n = int((~self.seen[k]).sum()) if k in self.seen else len(lattice_keys())
                if n:
                    out.append(k + ("%d lattice points" % n,))
                gone = set(space) - set(self.classes.get(k, {}))
                if gone:
                    out.append(k + ("%d classes" % len(gone),))
        return out


_SPACES = {}


def class_space(strength, floor):
    """{class key: lattice points in it}: the classes the lattice produces at this strength and division"""
    if (strength, floor) not in _SPACES:
        L = lattice()
        c, n = np.unique(class_key(classify(L, np.full(len(L), floor), strength)), return_counts=True)
        _SPACES[(strength, floor)] = dict(zip(c.tolist(), n.tolist()))
    return _SPACES[(strength, floor)]


# ---------------------------------------------------------------------------------------------------------------
# placement: the kernel's tiling, restated (csrc/post_kernel.inl)
# ---------------------------------------------------------------------------------------------------------------
TILE_KINDS = ("interior", "left", "right", "top", "bottom", "wrap", "trunc_cols", "trunc_rows", "chroma_limit")
TW, TH, OX = 128, 32, 124


def post_tile_columns(w):
    """(tile columns that run, wrap): post_tile_columns"""
    tiles = (w + OX + TW - 1) // TW
    spare = tiles * TW - OX - w
    wrap = 1 if (tiles >= 2 and w % 4 == 0 and spare >= 4) else 0
    return tiles - wrap, wrap


def tile_is_interior(w, h, sx, ty):
    """post_tile_is_interior_geom; also returns whether the luma conditions alone hold"""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    xl, yl = sx * TW - OX, ty * TH - 4
    w8, h8, cw8, ch8 = w // 8 * 8, h // 8 * 8, cw // 8 * 8, ch // 8 * 8
    luma = (xl >= 0) & (yl >= 0) & (xl + TW <= w8) & (yl + TH <= h8)
    # (C division of a negative xl / 2, yl / 2 truncates; xl, yl >= 0 is asked for anyway)
    chroma = (np.abs(xl) // 2 * np.sign(xl) + TW // 2 <= cw8) & (np.abs(yl) // 2 * np.sign(yl) + TH // 2 <= ch8)
    return luma & chroma, luma


def placement(w, h, plane, trace):
    """per quartet of a plane's trace: (half, kinds bool[n, len(TILE_KINDS)], sx, ty) -- the tile that filters it, by the
    strip arithmetic of post_phase_hedges / post_phase_vedges.  plane: 0 = Y, 1 / 2 = Cb / Cr; w, h: the LUMA size."""
    chroma = plane != 0
    pw, ph = ((w + 1) // 2, (h + 1) // 2) if chroma else (w, h)
    tiles_run, wrap = post_tile_columns(w)
    x, y, is_h = trace["x"].astype(np.int64), trace["y"].astype(np.int64), trace["dir"] == DIR_H
    sc = 2 if chroma else 1                                   # chroma strips are half the size
    riding = is_h & (wrap == 1) & (x < 4 // sc)
    sx = np.where(riding, tiles_run + wrap - 1, (x + OX // sc) // (TW // sc))
    # a horizontal edge's A row is 8e - 2: its strip is the one with the C row at its middle; a vertical edge's row y
    # lies in the strip that starts at 4 (mod 8) (chroma: 2 mod 4)
    sy = np.where(is_h, (y + 2) * sc // 8, (y + 4 // sc) // (8 // sc))
    ty = sy // 4
    xl, yl = sx * TW - OX, ty * TH - 4
    interior, luma_ok = tile_is_interior(w, h, sx, ty)
    kinds = np.zeros((len(trace), len(TILE_KINDS)), bool)
    kinds[:, 0] = interior
    kinds[:, 1] = xl < 0
    kinds[:, 2] = xl + TW > w
    kinds[:, 3] = yl < 0
    kinds[:, 4] = yl + TH > h
    kinds[:, 5] = riding
    kinds[:, 6] = is_h & (x >= pw // 8 * 8)
    kinds[:, 7] = ~is_h & (y >= ph // 8 * 8)
    kinds[:, 8] = luma_ok & ~interior
    half = np.where(is_h, x & 1, y & 1)
    return half, kinds, sx, ty


def geometry_exclusions(direction, kinds):
    """bool[n]: quartets that would sit in a combination the module docstring lists as empty (asserted none)"""
    k = {n: kinds[:, i] for i, n in enumerate(TILE_KINDS)}
    v = direction == DIR_V
    return (k["wrap"] & v) | (k["left"] & v) | (k["trunc_cols"] & v) | (k["trunc_rows"] & ~v) | \
        (k["interior"] & (k["trunc_cols"] | k["trunc_rows"]))


EXCLUDED_CELLS = {("wrap", DIR_V), ("left", DIR_V), ("trunc_cols", DIR_V), ("trunc_rows", DIR_H)}
CONDITIONS = ("d<0", "d>0", "ramp1", "ramp2", "ramp3", "d2 clipped", "saturated", "rounding-sensitive", "division-sensitive")


def conditions_of(cls):
    """bool[n, len(CONDITIONS)]"""
    return np.stack([cls["sign"] < 0, cls["sign"] > 0, cls["ramp"] == 1, cls["ramp"] == 2, cls["ramp"] == 3,
                     cls["d2clip"] == 2, cls["sat"] != 0, cls["roundsens"], ~cls["floor"] & (cls["divsens"] != 0)], axis=1)


def required_conditions(kind):
    """rounding-sensitive limits are asked of floor positions, division-sensitive numerators of truncation positions"""
    trunc = kind in ("trunc_cols", "trunc_rows")
    return [c for c in CONDITIONS if c != ("rounding-sensitive" if trunc else "division-sensitive")]


# ---------------------------------------------------------------------------------------------------------------
# table (b)
# ---------------------------------------------------------------------------------------------------------------
SIZES_B = [(384, 96), (388, 98), (390, 100), (392, 97), (384, 100), (390, 97)]
STRENGTHS_B = list(range(13)) * 2
# (Y, Cb, Cr) levels of a macroblock: near the ends of the byte range a sample still has to show in an unclamped channel
# (bt601.rs:25-58: R = 1.164 (Y - 16) + 1.596 (Cr - 128), B = 1.164 (Y - 16) + 2.018 (Cb - 128))
THEMES = [(249, 100, 96), (6, 128, 160), (6, 251, 128), (249, 4, 128), (40, 128, 251), (215, 128, 4), (128, 128, 128),
          (100, 150, 110), (170, 100, 150)]
THEME_WEIGHTS = [1, 1, 2, 2, 2, 2, 1, 1, 1]          # (a chroma plane has a quarter of the luma plane's quartets)
INTRA = 3
SEED_B = 0                # (any base will do as long as the classifier finds nothing missing: test_sim_post_sweep.py)


def picture_b(w, h, seed):
    """one seeded intra picture: (mbs, coeffs).  A chroma block whose theme puts it at an end of the range is either FLAT at
    254 / 1 or a trough / bowl (the coefficients (0, 2), (2, 0) or both) that clips at its rim and dips one sample inside:
    next to a flat neighbour that is A <= 247, B = 255 | 254, 254 and its mirror images, whose B + d1 or C - d1 leaves the byte
    range (a smoothing filter saturates on such overshoots only, never on a plain step)."""
    rng = np.random.default_rng(seed)
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    n = mbw * mbh
    mbs = np.zeros(n, MB_RECORD_DTYPE)
    mbs["mb_type"] = INTRA
    ti = rng.choice(len(THEMES), n, p=np.array(THEME_WEIGHTS) / sum(THEME_WEIGHTS))
    # (the picture's border macroblocks, where the rare tile kinds live, take the themes at the ends of the range only)
    border = np.zeros((mbh, mbw), bool)
    border[:, 0] = border[:, -2:] = border[-1, :] = True
    ti = np.where(border.ravel(), rng.integers(2, 6, n), ti)
    theme = np.array(THEMES)[ti]                                                   # [mb, plane]
    spread = rng.choice([3, 8, 24], n)
    levels = np.concatenate([np.repeat(theme[:, :1], 4, axis=1), theme[:, 1:]], axis=1)
    dc = np.clip(levels + rng.integers(-1, 2, (n, 6)) * spread[:, None] // 2 + rng.integers(-3, 4, (n, 6)), 1, 254)
    mbs["quant"] = rng.integers(1, 6, n)
    coded = rng.random((n, 6)) < 0.7
    cf = np.zeros((n, 6, 64), np.int16)
    reach = rng.choice([3, 8, 20, 40], (n, 6))                                     # (the widest ramps clip at the ends of the range)
    ii, bb = np.indices((n, 6))
    for k in range(3):                                                             # three low-frequency coefficients
        cf[ii, bb, rng.choice([1, 2, 8, 9, 16, 3, 24], (n, 6))] = rng.integers(-reach, reach + 1)
    cf[..., 1] += 2 * ~cf.any(axis=2)
    for blk, hi_theme, lo_theme in ((4, 2, 3), (5, 4, 5)):
        for th, sign in ((hi_theme, 1), (lo_theme, -1)):
            sel = np.flatnonzero(ti == th)
            flat = rng.random(sel.size) < 0.5
            dc[sel[flat], blk] = 254 if sign > 0 else 1
            coded[sel[flat], blk] = False
            bowl = sel[~flat]
            dc[bowl, blk] = (255 if sign > 0 else 0) - sign * rng.integers(20, 41, bowl.size)
            coded[bowl, blk] = True
            mbs["quant"][bowl] = 5
            cf[bowl, blk] = 0
            shape = rng.integers(0, 3, bowl.size)                                  # a trough along x, along y, or the bowl
            cf[bowl, blk, 2] = sign * rng.integers(20, 35, bowl.size) * (shape != 1)
            cf[bowl, blk, 16] = sign * rng.integers(20, 35, bowl.size) * (shape != 0)
    dc[dc == 128] = 129
    mbs["intradc"] = dc
    mbs["cbp"] = (coded * (1 << np.arange(6))).sum(axis=1)
    mbs["coeff_index"] = np.concatenate([[0], np.cumsum(coded.sum(axis=1))[:-1]])
    return mbs, np.ascontiguousarray(cf[coded])


def table_b():
    """dict(name, w, h, streams = [(mbs, coeffs)], strengths) per size"""
    for k, (w, h) in enumerate(SIZES_B):
        yield dict(name="b-%dx%d" % (w, h), w=w, h=h, strengths=list(STRENGTHS_B),
                   streams=[picture_b(w, h, SEED_B + 1000 * k + s) for s in range(len(STRENGTHS_B))])


def rgba_visibility(w, h, rgba):
    """per plane, bool[ph, pw]: the sample drives a channel that the RGBA (the oracle's, uint8[h * w * 4]) does not clamp"""
    px = np.asarray(rgba, np.uint8).reshape(h, w, 4)
    free = (px > 0) & (px < 255)
    cw, ch = (w + 1) // 2, (h + 1) // 2

    def quad_any(m):                                          # any pixel of the chroma sample's 2 x 2
        p = np.zeros((2 * ch, 2 * cw), bool)
        p[:h, :w] = m
        return p.reshape(ch, 2, cw, 2).any(axis=(1, 3))

    return free[:, :, :3].any(axis=2), quad_any(free[:, :, 2]), quad_any(free[:, :, 0])


class CoverageB:
    """the condition of table (b), counted twice: every quartet (plane outputs) and the RGBA-visible ones"""
    WAYS = ("planes", "rgba")

    def __init__(self):
        shape = (len(self.WAYS), len(TILE_KINDS), 3, 2, 2, len(CONDITIONS))
        self.count = np.zeros(shape, np.int64)
        self.quartets = np.zeros(shape[:-1], np.int64)
        self.excluded = 0
        self.unfiltered_ok = True

    def add_plane(self, w, h, plane, strength, trace, visible):
        """trace: this plane's (np_restatement.deblock_trace at `strength`); visible: rgba_visibility()[plane] of the
        oracle's RGBA of the FILTERED planes"""
        if not len(trace):
            return
        cls = classify(trace["abcd"], trace["floor"], strength)
        half, kinds, sx, ty = placement(w, h, plane, trace)
        self.excluded += int(geometry_exclusions(trace["dir"], kinds).sum())
        cond = conditions_of(cls)
        is_h = trace["dir"] == DIR_H
        x, y = trace["x"], trace["y"]
        vis = np.ones(len(trace), bool)
        for k in range(4):
            vis &= visible[np.where(is_h, y + k, y), np.where(is_h, x, x + k)]
        for wi, counted in enumerate((np.ones(len(trace), bool), vis)):
            for ki in range(len(TILE_KINDS)):
                for direction in (DIR_H, DIR_V):
                    for hf in (0, 1):
                        m = counted & kinds[:, ki] & (trace["dir"] == direction) & (half == hf)
                        if m.any():
                            self.quartets[wi, ki, plane, direction, hf] += int(m.sum())
                            self.count[wi, ki, plane, direction, hf] += cond[m].sum(axis=0)

    def add_picture(self, w, h, planes, strength, rgba):
        """planes: the oracle's decoded (unfiltered) planes of one stream; rgba: the oracle's RGBA of its filtered planes"""
        if strength == 0:
            return
        cw = (w + 1) // 2
        vis = rgba_visibility(w, h, rgba)
        for k, (p, pw) in enumerate(zip(planes, (w, cw, cw))):
            self.add_plane(w, h, k, strength, npr.deblock_trace(p, pw, strength)[2], vis[k])

    def missing(self):
        out = []
        for wi, way in enumerate(self.WAYS):
            for ki, kind in enumerate(TILE_KINDS):
                for plane in range(3):
                    for direction in (DIR_H, DIR_V):
                        if (kind, direction) in EXCLUDED_CELLS:
                            if self.quartets[wi, ki, plane, direction].sum():
                                out.append((way, kind, PLANE_NAMES[plane], DIR_NAMES[direction], "-", "excluded by geometry, yet not empty"))
                            continue
                        for hf in (0, 1):
                            for c in required_conditions(kind):
                                if not self.count[wi, ki, plane, direction, hf, CONDITIONS.index(c)]:
                                    out.append((way, kind, PLANE_NAMES[plane], DIR_NAMES[direction], hf, c))
        if self.excluded:
            out.append(("-", "-", "-", "-", "-", "%d quartets in combinations that geometry excludes" % self.excluded))
        return out

    def report(self):
        lines = []
        for wi, way in enumerate(self.WAYS):
            for ki, kind in enumerate(TILE_KINDS):
                q = self.quartets[wi, ki]
                lines.append("%-6s %-12s quartets Y %7d  Cb %6d  Cr %6d   saturated %5d  rounding-sensitive %6d  division-sensitive %6d"
                             % (way, kind, q[0].sum(), q[1].sum(), q[2].sum(), self.count[wi, ki, ..., 6].sum(),
                                self.count[wi, ki, ..., 7].sum(), self.count[wi, ki, ..., 8].sum()))
        return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------
# failure messages
# ---------------------------------------------------------------------------------------------------------------
def first_difference(name, path, w, h, got, want, source=None, strength=0):
    """None, or a sentence naming picture, path, plane, position, tile kind and the class of the quartet(s) that own the
    first differing byte.  got / want: (y, cb, cr) or a single luma plane; source: the unfiltered planes (for the trace)."""
    if not isinstance(got, (tuple, list)):
        got, want, source = (got,), (want,), (None if source is None else (source,))
    cw = (w + 1) // 2
    for k, (g, e) in enumerate(zip(got, want)):
        g, e = np.asarray(g).ravel(), np.asarray(e).ravel()
        if g.shape != e.shape:
            return "%s, %s, plane %s: %d bytes instead of %d" % (name, path, PLANE_NAMES[k], g.size, e.size)
        bad = np.flatnonzero(g != e)
        if not bad.size:
            continue
        pw = cw if k else w
        py, px = divmod(int(bad[0]), pw)
        msg = "%s, %s, plane %s, (x %d, y %d): got %d, expected %d; %d bytes differ" % (
            name, path, PLANE_NAMES[k], px, py, g[bad[0]], e[bad[0]], bad.size)
        if source is not None and strength:
            msg += describe_position(w, h, k, px, py, source[k], strength)
        return msg
    return None


def describe_position(w, h, plane, px, py, source_plane, strength):
    """'; <the quartets that own sample (px, py) of the plane, with tile, kinds and class>'"""
    pw = (w + 1) // 2 if plane else w
    t = npr.deblock_trace(source_plane, pw, strength)[2]
    own = np.where(t["dir"] == DIR_H, (t["x"] == px) & (t["y"] <= py) & (py < t["y"] + 4),
                   (t["y"] == py) & (t["x"] <= px) & (px < t["x"] + 4))
    if not own.any():
        return "; no quartet filters this byte"
    t = t[own]
    cls = classify(t["abcd"], t["floor"], strength)
    half, kinds, sx, ty = placement(w, h, plane, t)
    msg = ""
    for i in range(len(t)):
        msg += "; %s quartet %s of plane %s at (x %d, y %d), half %d, tile (%d, %d) [%s]: %s" % (
            DIR_NAMES[t["dir"][i]], t["abcd"][i].tolist(), PLANE_NAMES[plane], t["x"][i], t["y"][i], half[i], sx[i], ty[i],
            ", ".join(n for n, on in zip(TILE_KINDS, kinds[i]) if on) or "general", describe_class(cls[i]))
    return msg


def rgba_difference(name, path, w, h, got, want, source=None, strength=0):
    """first_difference for an RGBA picture (w * h * 4 bytes): the pixel, and the quartets of its three samples"""
    g, e = np.asarray(got).ravel(), np.asarray(want).ravel()
    if g.shape != e.shape:
        return "%s, %s: %d RGBA bytes instead of %d" % (name, path, g.size, e.size)
    bad = np.flatnonzero(g != e)
    if not bad.size:
        return None
    py, px = divmod(int(bad[0]) // 4, w)
    msg = "%s, %s, RGBA pixel (x %d, y %d): got %s, expected %s; %d bytes differ" % (
        name, path, px, py, g[bad[0] // 4 * 4:bad[0] // 4 * 4 + 4].tolist(), e[bad[0] // 4 * 4:bad[0] // 4 * 4 + 4].tolist(), bad.size)
    if source is not None and strength:
        for k in range(3):
            msg += describe_position(w, h, k, px // 2 if k else px, py // 2 if k else py, source[k], strength)
    return msg
