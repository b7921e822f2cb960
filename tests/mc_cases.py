"""Designed motion-compensation cases and the accounting of what they exercise.

INPUTS ONLY: this file builds macroblock records (for H263State.submit_picture, Batch.decode, simlib.recon and the
oracles) and reference-picture inputs.  Expected pixels never come from here -- they are the C oracle's, cross-checked
by oracle/np_restatement.py.

The tables (one generator each, yielding dicts with table / w / h / mbs / coeffs / tag):
  (a) table_a   every plane width 1..80 (+ 128, 1920: width == row pitch), every block column, every tap-window start
                u from 10 left of the plane to 2 right of its last pixel, ix 0 / 1, two vertical situations -- luma
                through 4MV macroblocks, chroma through the vector derived from a one-vector macroblock
  (b) table_b   picture heights 1..40, every piece row group, every v from 6 above the plane to 2 below its last row,
                iy 0 / 1, six horizontal situations (inside at each u & 3, left border, right border)
  (c) table_c   {left-out, left-straddle, right-straddle, right-out} x {top-out, ..., bottom-out} x ix x iy at plane
                widths of every residue mod 4 below and above 9
  (d) table_d   waves whose eight macroblocks all carry integer vectors (the kernel's short cut), with every u & 3,
                border lanes next to inside lanes, intra and invalid macroblocks in the wave, and the two mixed cases
  (e) table_e   4MV macroblocks of four different vectors whose i16 component sum takes every value that leaves the
                chroma block inside a 1920-wide plane; table_e_wrap: sums that leave the i16 range and wrap
  (f) table_f   the reference planes in which every pair of two-tap sums occurs, and the three half-pel pictures

Coverage is the classifier's business: it works from the records alone, with the rules the kernel applies
(u = px + (mvx >> 1), ix = mvx & 1, inside = 0 <= u <= pw - 8 - ix, the ballot over the 64 lanes of a wave in which a
lane that takes no prediction counts as vector 0).  The tests assert that nothing of a declared space is missing.
"""
import numpy as np

from oracle.oracle import MB_RECORD_DTYPE

INTER, INTER4V, INTRA = 0, 2, 3
NO_COEFFS = np.zeros((0, 64), np.int16)


def mb_dims(w, h):
    return (w + 15) // 16, (h + 15) // 16


def _blank(w, h):
    mbw, mbh = mb_dims(w, h)
    m = np.zeros((mbh, mbw), MB_RECORD_DTYPE)
    m["quant"] = 1
    return m


def _pic(table, w, h, m, coeffs=None, **tag):
    return {"table": table, "w": w, "h": h, "mbs": np.ascontiguousarray(m.ravel()),
            "coeffs": NO_COEFFS if coeffs is None else coeffs, "tag": tag}


def reference_records(w, h):
    """The I picture whose decoded planes are the reference of every case of that size: a key frame is the only way a
    reference gets into a decoder.  INTRADC everywhere plus a few coefficients per block, so that neighbouring pixels
    differ (a flat reference would hide a wrong tap).  Returns (mbs, coeffs)."""
    rng = np.random.default_rng(w * 65537 + h)
    mbw, mbh = mb_dims(w, h)
    n = mbw * mbh
    mbs = np.zeros(n, MB_RECORD_DTYPE)
    mbs["mb_type"] = INTRA
    mbs["quant"] = rng.integers(4, 12, n)
    dc = rng.integers(40, 216, (n, 6))
    dc[dc == 128] = 129
    mbs["intradc"] = dc
    mbs["cbp"] = 0x3F
    mbs["coeff_index"] = np.arange(n) * 6
    co = np.zeros((n * 6, 64), np.int16)
    for _ in range(6):                                           # up to six coefficients among the 20 lowest raster positions
        pos = rng.choice(np.array([1, 2, 3, 4, 8, 9, 10, 11, 16, 17, 18, 24, 25, 5, 12, 19, 26, 32, 33, 40]), n * 6)
        co[np.arange(n * 6), pos] = rng.integers(-12, 13, n * 6)
    return mbs, co


def chroma_component(c):
    """the component of a ONE-vector macroblock whose derived chroma component is c (sum = 4 mv: 8c -> c for an even c,
    16j + 4 -> 2j + 1 for c = 2j + 1; types.rs:759-768)"""
    c = np.asarray(c)
    return np.where(c % 2 == 0, 2 * c, 2 * c - 1)


def chroma_vectors(mv):
    """(..., 4, 2) luma vectors -> (..., 2) chroma vectors by the kernel's rule: the i16 (wrapping) sum s, then
    ((s >> 4) << 1) + (frac > 2) + (frac >= 14)"""
    s = np.asarray(mv, np.int64).sum(axis=-2)
    s = ((s + 32768) % 65536) - 32768
    frac = s & 15
    return ((s >> 3) & ~1) + ((frac + 13) >> 4) + ((frac + 2) >> 4)


def with_residual_and_intra(pic, seed):
    """a copy of a picture in which some macroblocks are intra (the prediction's `keep` mask) and some inter macroblocks
    carry a small residual -- EXTRA pictures: the coverage of the plain one is not taken away"""
    rng = np.random.default_rng(seed)
    m = pic["mbs"].copy()
    n = len(m)
    kind = rng.integers(0, 6, n)                                # 0: intra, 1: residual, else unchanged
    coeffs = []
    for i in range(n):
        if kind[i] == 0:
            m[i]["mb_type"] = INTRA
            m[i]["mv"] = 0
            m[i]["intradc"] = rng.integers(1, 128, 6)
        elif kind[i] == 1:
            m[i]["quant"] = 10
            m[i]["cbp"] = int(rng.integers(1, 64))
            m[i]["coeff_index"] = len(coeffs)
            for _ in range(bin(int(m[i]["cbp"])).count("1")):
                c = np.zeros(64, np.int16)
                c[rng.choice(np.array([0, 1, 8, 9, 2, 16]), 3, replace=False)] = rng.integers(-6, 7, 3)
                coeffs.append(c)
    co = np.array(coeffs, np.int16).reshape(-1, 64) if coeffs else NO_COEFFS
    return {"table": pic["table"], "w": pic["w"], "h": pic["h"], "mbs": m, "coeffs": co,
            "tag": dict(pic["tag"], variant="residual+intra")}


# ---------------------------------------------------------------------------------------------------------------
# (a) horizontal table
# ---------------------------------------------------------------------------------------------------------------
A_WIDTHS = tuple(range(1, 81)) + (128, 1920)
A_U_LEFT, A_U_RIGHT = 10, 2                                     # u from -10 to pw + 1


def a_rows(W):
    """the macroblock-row specifications of width W: ('Y', u, ix) sweeps every luma block column (block row 0 with
    iy = 0, block row 1 with iy = 1), ('C', u, ix, iy) every chroma block column"""
    cw = (W + 1) // 2
    rows = [("Y", u, ix, None) for ix in (0, 1) for u in range(-A_U_LEFT, W + A_U_RIGHT)]
    rows += [("C", u, ix, iy) for iy in (0, 1) for ix in (0, 1) for u in range(-A_U_LEFT, cw + A_U_RIGHT)]
    return rows


def a_height(W):
    return 16 * (8 if W <= 128 else 68)


def _picture_a(W, H, rows):
    m = _blank(W, H)
    mbw, mbh = mb_dims(W, H)
    mbx = np.arange(mbw)
    for r, (kind, u, ix, iy) in enumerate(rows):
        if kind == "Y":
            m["mb_type"][r] = INTER4V
            for b in range(4):
                m["mv"][r, :, b, 0] = 2 * (u - 8 * (2 * mbx + (b & 1))) + ix
                m["mv"][r, :, b, 1] = 0 if b < 2 else -1       # block row 1: v = py + 8 - 1, iy = 1 (inside)
        else:
            m["mb_type"][r] = INTER
            cy = 0 if iy == 0 else (1 if r + 1 < mbh else -1)   # (the last row looks up, the others down: inside)
            m["mv"][r, :, :, 0] = chroma_component(2 * (u - 8 * mbx) + ix)[:, None]
            m["mv"][r, :, :, 1] = chroma_component(cy)
    return _pic("a", W, H, m, width=W)


def table_a(widths=A_WIDTHS):
    for W in widths:
        rows, H = a_rows(W), a_height(W)
        R = H // 16
        for i in range(0, len(rows), R):
            chunk = rows[i:i + R]
            chunk = chunk + rows[:R - len(chunk)]               # (the last picture is filled up from the start)
            pic = _picture_a(W, H, chunk)
            yield pic
            if i == 0 and W in (16, 33, 47, 80, 128):
                yield with_residual_and_intra(pic, W)


# ---------------------------------------------------------------------------------------------------------------
# (b) vertical table
# ---------------------------------------------------------------------------------------------------------------
B_HEIGHTS = tuple(range(1, 41))
B_WIDTH = 96                                                    # 12 luma / 6 chroma block columns: the six situations
B_V_ABOVE, B_V_BELOW = 6, 2                                     # v from -6 to ph + 1
H_INSIDE0, H_LEFT, H_RIGHT = 0, 4, 5                            # situations 0..3 = inside with u & 3


def _b_u(col, pw):
    """window start of block column `col` in situation col % 6"""
    hs = col % 6
    return -3 if hs == H_LEFT else (pw - 5 if hs == H_RIGHT else 8 * col + hs)


def table_b(heights=B_HEIGHTS, thin=1):
    """thin > 1 keeps every thin-th v of the interior of the sweep (the values within 12 rows of either end stay)"""
    W = B_WIDTH
    for ph in heights:
        mbw, mbh = mb_dims(W, ph)
        mby, mbx = np.divmod(np.arange(mbw * mbh), mbw)
        mby, mbx = mby.reshape(mbh, mbw), mbx.reshape(mbh, mbw)
        cph = (ph + 1) // 2

        def kept(t, lo, hi):
            return thin == 1 or t - lo < 12 or hi - t < 12 or (t - lo) % thin == 0

        for iy in (0, 1):
            # luma: every block at the absolute row t (pieces at t and t + 4)
            for t in range(-B_V_ABOVE - 4, ph + B_V_BELOW):
                if not kept(t, -B_V_ABOVE - 4, ph + B_V_BELOW - 1):
                    continue
                m = _blank(W, ph)
                m["mb_type"] = INTER4V
                for b in range(4):
                    col = 2 * mbx + (b & 1)
                    u = np.vectorize(_b_u)(col, W)
                    m["mv"][:, :, b, 0] = 2 * (u - 8 * col) + ((col // 6) & 1)
                    m["mv"][:, :, b, 1] = 2 * (t - (16 * mby + 8 * (b >> 1))) + iy
                yield _pic("b", W, ph, m, plane="Y", v=t, iy=iy)
            # chroma: the derived vector puts every block at the absolute row t (pieces at t, t + 2, t + 4, t + 6)
            for t in range(-B_V_ABOVE - 6, cph + B_V_BELOW):
                if not kept(t, -B_V_ABOVE - 6, cph + B_V_BELOW - 1):
                    continue
                m = _blank(W, ph)
                m["mb_type"] = INTER
                u = np.vectorize(_b_u)(mbx, W // 2)
                m["mv"][:, :, :, 0] = chroma_component(2 * (u - 8 * mbx) + (t & 1))[:, :, None]
                m["mv"][:, :, :, 1] = chroma_component(2 * (t - 8 * mby) + iy)[:, :, None]
                yield _pic("b", W, ph, m, plane="C", v=t, iy=iy)
        if ph in (7, 16, 33):
            yield with_residual_and_intra(_pic("b", W, ph, m, plane="C"), ph)


# ---------------------------------------------------------------------------------------------------------------
# (c) corners
# ---------------------------------------------------------------------------------------------------------------
C_WIDTHS = (5, 6, 7, 8, 20, 21, 22, 23)                         # plane widths: every residue mod 4 below and above 9
C_HEIGHTS = (7, 22)
OUT_LOW, STRADDLE_LOW, STRADDLE_HIGH, OUT_HIGH = range(4)       # left / top ... right / bottom


def _c_start(sit, extent):
    return (-12, -3, extent - 4, extent + 3)[sit]


def table_c(widths=C_WIDTHS, heights=C_HEIGHTS, situations=None):
    """situations: None = the whole cross product, else an iterable of (hs, vs, ix, iy)"""
    sits = situations or [(hs, vs, ix, iy) for hs in range(4) for vs in range(4) for ix in (0, 1) for iy in (0, 1)]
    for pw in widths:
        for ph in heights:
            for plane in "YC":
                W, H = (pw, ph) if plane == "Y" else (2 * pw, 2 * ph)
                mbw, mbh = mb_dims(W, H)
                mby, mbx = np.divmod(np.arange(mbw * mbh), mbw)
                mby, mbx = mby.reshape(mbh, mbw), mbx.reshape(mbh, mbw)
                for hs, vs, ix, iy in sits:
                    u, v = _c_start(hs, pw), _c_start(vs, ph)
                    m = _blank(W, H)
                    if plane == "Y":                            # every block lands on the same window
                        m["mb_type"] = INTER4V
                        for b in range(4):
                            m["mv"][:, :, b, 0] = 2 * (u - (16 * mbx + 8 * (b & 1))) + ix
                            m["mv"][:, :, b, 1] = 2 * (v - (16 * mby + 8 * (b >> 1))) + iy
                    else:
                        m["mb_type"] = INTER
                        m["mv"][:, :, :, 0] = chroma_component(2 * (u - 8 * mbx) + ix)[:, :, None]
                        m["mv"][:, :, :, 1] = chroma_component(2 * (v - 8 * mby) + iy)[:, :, None]
                    yield _pic("c", W, H, m, plane=plane, hs=hs, vs=vs, ix=ix, iy=iy)


# ---------------------------------------------------------------------------------------------------------------
# (d) whole-wave integer vectors
# ---------------------------------------------------------------------------------------------------------------
D_WIDTHS = (128, 176, 48, 104)          # 8 macroblocks (width == pitch), 11 (a second wave of 3), 3 and 7 (narrow pictures)
D_HEIGHT = 32


def _d_integer_vectors(sh_luma, sh_chroma, mbw, borders):
    """(mbw, 4, 2) even vectors: every luma window starts at u & 3 == sh_luma, every derived chroma vector is even
    with u & 3 == sh_chroma; borders: the first macroblock looks left of the picture, the last one right of it"""
    mv = np.zeros((mbw, 4, 2), np.int64)
    for x in range(mbw):
        # luma displacements dx_i = sh + 4 a_i with sum(a) == sh (mod 2): the component sum 2 sum(dx) is 0 (mod 16)
        a = np.array([0, 1, -1, sh_luma & 1])
        dx = sh_luma + 4 * a
        # the chroma displacement is sum(2 dx) / 16; adding 8 m to one luma displacement adds m to it
        cd = int((2 * dx).sum()) // 16
        dx[x % 3] += 8 * ((sh_chroma - cd) % 4)
        if borders and x == 0:
            dx -= 16 * 4                                        # (a multiple of 16: both u & 3 stay)
        if borders and x == mbw - 1:
            dx += 16 * 4
        mv[x, :, 0] = 2 * dx
        mv[x, :, 1] = (4, -4, 0, 0) if x & 1 else (0, 0, 0, 0)
    return mv


def table_d(widths=D_WIDTHS):
    H = D_HEIGHT
    for W in widths:
        mbw, mbh = mb_dims(W, H)
        for sh in range(4):
            for shc in range(4):
                for borders in (False, True):
                    for intra in (False, True):
                        if intra and (shc != sh):
                            continue
                        m = _blank(W, H)
                        m["mb_type"] = INTER4V
                        m["mv"] = _d_integer_vectors(sh, shc, mbw, borders)[None]
                        co = None
                        if intra:                               # an intra macroblock in the wave: all_inter is false
                            k = 1 if mbw > 2 else 0
                            m["mb_type"][:, k] = INTRA
                            m["mv"][:, k] = 0
                            m["intradc"][:, k] = 77
                        yield _pic("d", W, H, m, co, sh=sh, sh_chroma=shc, borders=borders, intra=intra)
        # the two mixed cases, with every u & 3 of the integer plane
        for sh in range(4):
            m = _blank(W, H)                                    # luma integer, chroma not: one vector 2 dx, dx odd -> frac 8
            m["mb_type"] = INTER
            dx = np.array([2 * (x % 5) + 1 + (sh & 2) for x in range(mbw)])
            m["mv"][:, :, :, 0] = (2 * dx)[None, :, None]
            m["mv"][0, :, :, 1] = 2
            m["mv"][1, :, :, 1] = -6
            yield _pic("d", W, H, m, mixed="luma")
            m = _blank(W, H)                                    # chroma integer, luma not: 16 k + (1, -1, 0, 0)
            m["mb_type"] = INTER4V
            m["mv"][:, :, :, 0] = (8 * sh + np.array([1, -1, 0, 0]))[None, None, :]
            m["mv"][:, :, :, 1] = np.array([0, 1, -1, 0])[None, None, :]
            yield _pic("d", W, H, m, mixed="chroma")


# ---------------------------------------------------------------------------------------------------------------
# (e) chroma vector: every component sum
# ---------------------------------------------------------------------------------------------------------------
E_WIDTH, E_HEIGHT = 1920, 256                                   # chroma plane 960 x 128; 120 x 16 macroblocks


def _e_inside_sums(n_blocks, plane_extent):
    """{block index: the sums s whose derived component keeps that block's window inside the plane}, over every i16 s;
    the sums are dealt evenly to the blocks (about 256 each)"""
    s = np.arange(-32768, 32768)
    c = chroma_vectors(np.stack([s, 0 * s, 0 * s, 0 * s], axis=-1)[..., None])[..., 0]
    d, i = c >> 1, c & 1
    lo, hi = -d, plane_extent - 8 - i - d                       # 8 * block must lie in [lo, hi]
    blk = np.clip((plane_extent - 8 - d) // 16, 0, n_blocks - 1)    # 8 * blk + d is about half way between d and the far end
    blk = np.where(8 * blk < lo, blk + 1, blk)
    ok = (8 * blk >= lo) & (8 * blk <= hi) & (blk >= 0) & (blk < n_blocks)
    return {b: s[ok & (blk == b)] for b in range(n_blocks)}


def e_declared(n_blocks, plane_extent):
    """every sum for which SOME block of the row / column keeps its window inside the plane"""
    s = np.arange(-32768, 32768)
    c = chroma_vectors(np.stack([s, 0 * s, 0 * s, 0 * s], axis=-1)[..., None])[..., 0]
    d, i = c >> 1, c & 1
    first = np.maximum(0, -(d // 8))                            # smallest block with 8 * block + d >= 0
    return s[(first < n_blocks) & (8 * first + d <= plane_extent - 8 - i)]


def _four_vectors(s):
    """four DIFFERENT i16 numbers whose sum is s"""
    s = np.asarray(s, np.int64)
    q = s >> 2
    return np.stack([q - 5, q - 2, q + 3, s - (3 * q - 4)], axis=-1)


def table_e():
    W, H = E_WIDTH, E_HEIGHT
    mbw, mbh = mb_dims(W, H)
    by_col = _e_inside_sums(mbw, W // 2)
    by_row = _e_inside_sums(mbh, H // 2)
    n_pictures = (max(len(v) for v in by_col.values()) + mbh - 1) // mbh
    for p in range(n_pictures):
        m = _blank(W, H)
        m["mb_type"] = INTER4V
        for r in range(mbh):
            k = p * mbh + r                                     # the k-th sum of every column's list
            sx = np.array([by_col[c][k % len(by_col[c])] for c in range(mbw)])
            j = p * mbw + np.arange(mbw)                        # ... and the j-th of this row's list
            sy = by_row[r][j % len(by_row[r])]
            m["mv"][r, :, :, 0] = _four_vectors(sx)
            m["mv"][r, :, :, 1] = _four_vectors(sy)[:, ::-1]
        yield _pic("e", W, H, m, picture=p)


def table_e_wrap():
    """component sums that leave the i16 range: four vectors near +-16384 whose sum wraps to a small number put the chroma
    block inside the picture while every luma tap clamps to the picture's edge"""
    W, H = 64, 48
    mbw, mbh = mb_dims(W, H)
    for sign in (1, -1):
        for comp in (0, 1):
            m = _blank(W, H)
            m["mb_type"] = INTER4V
            k = np.arange(mbw * mbh).reshape(mbh, mbw)
            small = (k * 7) % 23 - 11                           # the wrapped sum: -11 .. 11, both parities, fractions of all kinds
            m["mv"][:, :, :, comp] = sign * 16384 + np.array([-500, -200, 300, 400])[None, None, :]
            m["mv"][:, :, 3, comp] += small                     # the true sum is +-65536 + small
            m["mv"][:, :, :, 1 - comp] = np.array([1, 0, -1, 2])[None, None, :]
            yield _pic("e'", W, H, m, sign=sign, component=comp)


# ---------------------------------------------------------------------------------------------------------------
# (f) every pair of two-tap sums
# ---------------------------------------------------------------------------------------------------------------
F_LUMA, F_CHROMA = 528, 264


def f_plane(n):
    """n x n samples: row 0 is p[i] = (i mod 512) // 2 -- adjacent sums take every value 0..510 --, row j the same pattern
    rotated by o_j, o_(j+1) = o_j + j + 1 (mod 512): the offset between neighbouring rows takes every value"""
    j = np.arange(n)
    o = (j * (j + 1) // 2) % 512
    return ((((np.arange(n)[None, :] - o[:, None]) % 512) // 2)).astype(np.uint8)


def f_reference_planes():
    y, c = f_plane(F_LUMA), f_plane(F_CHROMA)
    return y.ravel(), c.ravel(), np.ascontiguousarray(c[::-1]).ravel()


def pair_coverage(plane):
    """bool[511, 511]: [a, b] is set when some pixel's upper two-tap sum is a and its lower one b"""
    p = np.asarray(plane, np.int32)
    s = p[:, :-1] + p[:, 1:]
    seen = np.zeros((511, 511), bool)
    seen[s[:-1].ravel(), s[1:].ravel()] = True
    return seen


def sum_coverage(plane):
    """(bool[511] of the horizontal two-tap sums, bool[511] of the vertical ones)"""
    p = np.asarray(plane, np.int32)
    hs, vs = np.zeros(511, bool), np.zeros(511, bool)
    hs[(p[:, :-1] + p[:, 1:]).ravel()] = True
    vs[(p[:-1] + p[1:]).ravel()] = True
    return hs, vs


F_VECTORS = ((1, 1), (1, 0), (0, 1))


def table_f(size=F_LUMA):
    """one vector on every macroblock: (+1/2, +1/2), x only, y only (the derived chroma vector is the same half-pel)"""
    for mvx, mvy in F_VECTORS:
        m = _blank(size, size)
        m["mb_type"] = INTER
        m["mv"][..., 0] = mvx
        m["mv"][..., 1] = mvy
        yield _pic("f", size, size, m, vector=(mvx, mvy))


def f_blocks_reference():
    """The planes of (f) with every sample blown up to a flat 8x8 block (4224 x 4224 luma): what a decoder can be made to
    hold, since a reference only ever gets there by being decoded -- INTRADC alone gives a block any flat value 1..254,
    and a second picture pushes 1 -> 0 and 254 -> 255.  The pair of sums of a sample quadruple then sits at the corner
    where its four blocks meet.  Returns (w, h, intra records, push records, push coefficients)."""
    n = F_CHROMA                                                # macroblocks per row and column
    y, c = f_plane(F_LUMA).astype(np.int64), f_plane(F_CHROMA).astype(np.int64)
    vals = np.zeros((n, n, 6), np.int64)
    for b in range(4):
        vals[:, :, b] = y[(b >> 1)::2, (b & 1)::2]
    vals[:, :, 4], vals[:, :, 5] = c, c[::-1]
    vals = vals.reshape(n * n, 6)
    intra = np.zeros(n * n, MB_RECORD_DTYPE)
    intra["mb_type"] = INTRA
    intra["quant"] = 1
    code = np.clip(vals, 1, 254)
    code[vals == 128] = 255                                     # (code 255 is level 1024: 128)
    intra["intradc"] = code
    push = np.zeros(n * n, MB_RECORD_DTYPE)
    push["quant"] = 1
    ends = (vals == 0) | (vals == 255)
    push["cbp"] = (ends * (1 << np.arange(6))).sum(axis=1)
    push["coeff_index"] = np.cumsum(ends.sum(axis=1)) - ends.sum(axis=1)
    co = np.zeros((int(ends.sum()), 64), np.int16)
    co[:, 0] = np.where(vals[ends] == 0, -4, 4)                 # quantiser 1: +-9 -> a flat residual of +-1
    return 8 * F_LUMA, 8 * F_LUMA, intra, push, co


# ---------------------------------------------------------------------------------------------------------------
# the classifier
# ---------------------------------------------------------------------------------------------------------------
def _corner(start, n_taps, extent):
    last = start + n_taps - 1
    return np.where(last < 0, OUT_LOW, np.where(start < 0, STRADDLE_LOW, np.where(start > extent - 1, OUT_HIGH,
                    np.where(last > extent - 1, STRADDLE_HIGH, -1))))


class Coverage:
    """what a set of pictures exercises, computed from their records alone"""

    def __init__(self):
        self.a, self.b, self.c = {}, {}, {}
        self.d = set()
        self.e = {0: np.zeros(65536, bool), 1: np.zeros(65536, bool)}
        self.e_wrap = set()

    # ---- the records as the kernel sees them
    @staticmethod
    def planes(pic):
        w, h = pic["w"], pic["h"]
        mbw, mbh = mb_dims(w, h)
        n = mbw * mbh
        mbs = np.zeros(n, MB_RECORD_DTYPE)
        mbs[:len(pic["mbs"])] = pic["mbs"]
        inter = np.isin(mbs["mb_type"], (0, 1, 2, 5))
        mby, mbx = np.divmod(np.arange(n), mbw)
        mv = mbs["mv"].astype(np.int64) * inter[:, None, None]            # a lane without a prediction counts as vector 0
        cmv = chroma_vectors(mv)
        off = np.arange(4)
        Y = {"kind": "Y", "pw": w, "ph": h, "px": 16 * mbx[:, None] + 8 * (off & 1), "py": 16 * mby[:, None] + 8 * (off >> 1),
             "mvx": mv[:, :, 0], "mvy": mv[:, :, 1], "pred": np.repeat(inter[:, None], 4, 1), "rows": 4, "pieces": 2}
        Cc = {"kind": "C", "pw": (w + 1) // 2, "ph": (h + 1) // 2, "px": 8 * mbx[:, None], "py": 8 * mby[:, None],
              "mvx": cmv[:, None, 0], "mvy": cmv[:, None, 1], "pred": inter[:, None], "rows": 2, "pieces": 4}
        return mbs, inter, mv, (Y, Cc)

    def add(self, pic):
        mbs, inter, mv, planes = self.planes(pic)
        for P in planes:
            kind, pw, ph = P["kind"], P["pw"], P["ph"]
            ix, iy = P["mvx"] & 1, P["mvy"] & 1
            u, v = P["px"] + (P["mvx"] >> 1), P["py"] + (P["mvy"] >> 1)
            pred = P["pred"]
            inside_h = (u >= 0) & (u <= pw - 8 - ix)
            inside_v = (v >= 0) & (v <= ph - 8 - iy)
            # (a): block column x window start x ix x iy, vertically inside
            sel = pred & inside_v & (u >= -A_U_LEFT) & (u <= pw + A_U_RIGHT - 1) & (P["px"] < pw)
            if sel.any():
                t = self.a.setdefault((kind, pw), np.zeros(((pw + 7) // 8, pw + A_U_LEFT + A_U_RIGHT, 2, 2), bool))
                t[(P["px"] // 8)[sel], (u + A_U_LEFT)[sel], ix[sel], iy[sel]] = True
            # (b): row group x piece row x iy x horizontal situation
            hs = np.where(u < 0, H_LEFT, np.where(u > pw - 8 - ix, H_RIGHT, u & 3))
            tb = self.b.setdefault((kind, ph), np.zeros(((ph + P["rows"] - 1) // P["rows"], ph + B_V_ABOVE + B_V_BELOW, 2, 6), bool))
            for k in range(P["pieces"]):
                py, vp = P["py"] + P["rows"] * k, v + P["rows"] * k
                sel = pred & (py < ph) & (vp >= -B_V_ABOVE) & (vp <= ph + B_V_BELOW - 1)
                tb[(py // P["rows"])[sel], (vp + B_V_ABOVE)[sel], iy[sel], hs[sel]] = True
            # (c): corners
            ch, cv = _corner(u, 8 + ix, pw), _corner(v, 8 + iy, ph)
            sel = pred & (ch >= 0) & (cv >= 0)
            if sel.any():
                tc = self.c.setdefault((kind, pw, ph), np.zeros((4, 4, 2, 2), bool))
                tc[ch[sel], cv[sel], ix[sel], iy[sel]] = True
        self._add_waves(pic, mbs, inter, mv, planes)
        self._add_sums(pic, mbs, inter, planes)

    def _add_waves(self, pic, mbs, inter, mv, planes):
        """(d): per wave of eight macroblocks of a row, the kernel's two ballots"""
        mbw, mbh = mb_dims(pic["w"], pic["h"])
        Y, Cc = planes
        coded = mbs["cbp"] != 0
        for mby in range(mbh):
            for x0 in range(0, mbw, 8):
                idx = mby * mbw + np.arange(x0, min(x0 + 8, mbw))
                valid_all = len(idx) == 8
                it = inter[idx]
                if not it.any():
                    continue                                    # nothing is predicted: the MC = false form
                if valid_all and it.all() and not coded[idx].any() and not mv[idx].any():
                    continue                                    # the static short cut: a copy
                integer = {}
                for P in (Y, Cc):
                    integer[P["kind"]] = not ((P["mvx"][idx] | P["mvy"][idx]) & 1).any()
                if integer["Y"] != integer["C"]:
                    self.d.add(("mixed", "Y" if integer["Y"] else "C"))
                for P in (Y, Cc):
                    if not integer[P["kind"]]:
                        continue
                    k = P["kind"]
                    u = (P["px"] + (P["mvx"] >> 1))[idx]
                    pred = P["pred"][idx]
                    inside = pred & (u >= 0) & (u <= P["pw"] - 8)
                    left, right = pred & (u < 0), pred & (u > P["pw"] - 8)
                    for s in np.unique(u[inside] & 3):
                        self.d.add((k, "sh", int(s)))
                    if inside.any() and left.any():
                        self.d.add((k, "left+inside"))
                    if inside.any() and right.any():
                        self.d.add((k, "right+inside"))
                    if valid_all and not it.all():
                        self.d.add((k, "intra"))
                    if not valid_all:
                        self.d.add((k, "invalid"))
                    if valid_all and it.all():
                        self.d.add((k, "all_inter"))

    def _add_sums(self, pic, mbs, inter, planes):
        """(e): the i16 component sums of 4MV macroblocks with four different vectors whose chroma block is inside"""
        if pic["w"] != E_WIDTH and pic["table"] != "e'":
            return
        Cc = planes[1]
        mvr = mbs["mv"].astype(np.int64)
        distinct = np.ones(len(mbs), bool)
        for i in range(4):
            for j in range(i):
                distinct &= (mvr[:, i] != mvr[:, j]).any(axis=1)
        raw = mvr.sum(axis=1)
        s = ((raw + 32768) % 65536) - 32768
        ix, iy = Cc["mvx"][:, 0] & 1, Cc["mvy"][:, 0] & 1
        u, v = Cc["px"][:, 0] + (Cc["mvx"][:, 0] >> 1), Cc["py"][:, 0] + (Cc["mvy"][:, 0] >> 1)
        in_h = (u >= 0) & (u <= Cc["pw"] - 8 - ix)
        in_v = (v >= 0) & (v <= Cc["ph"] - 8 - iy)
        ok = inter & distinct & (mbs["mb_type"] == INTER4V)
        if pic["w"] == E_WIDTH:
            self.e[0][(s[:, 0] + 32768)[ok & in_h]] = True
            if pic["h"] == E_HEIGHT:
                self.e[1][(s[:, 1] + 32768)[ok & in_v]] = True
        for comp, inside in ((0, in_h), (1, in_v)):
            wrapped = ok & inside & (raw[:, comp] != s[:, comp])
            for sign in (1, -1):
                if (wrapped & (np.sign(raw[:, comp]) == sign)).any():
                    self.e_wrap.add((sign, comp))

    # ---- what is missing from the declared spaces
    def missing_a(self, widths=A_WIDTHS):
        out = []
        for W in widths:
            for kind, pw in (("Y", W), ("C", (W + 1) // 2)):
                t = self.a.get((kind, pw))
                if t is None:
                    out.append((kind, pw, "nothing"))
                    continue
                for col, uu, ix, iy in np.argwhere(~t)[:20]:
                    out.append((kind, pw, int(col), int(uu) - A_U_LEFT, int(ix), int(iy)))
        return out

    def missing_b(self, heights=B_HEIGHTS):
        out = []
        for ph in sorted(set(heights) | set((p + 1) // 2 for p in heights)):
            for kind in ("Y", "C"):
                if kind == "Y" and ph not in heights:
                    continue
                if kind == "C" and ph not in set((p + 1) // 2 for p in heights):
                    continue
                t = self.b.get((kind, ph))
                if t is None:
                    out.append((kind, ph, "nothing"))
                    continue
                for g, vv, iy, hs in np.argwhere(~t)[:20]:
                    out.append((kind, ph, int(g), int(vv) - B_V_ABOVE, int(iy), int(hs)))
        return out

    def missing_c(self, widths=C_WIDTHS, heights=C_HEIGHTS, situations=None):
        want = np.zeros((4, 4, 2, 2), bool)
        if situations is None:
            want[:] = True
        else:
            for s in situations:
                want[s] = True
        out = []
        for kind in "YC":
            for pw in widths:
                for ph in heights:
                    t = self.c.get((kind, pw, ph), np.zeros((4, 4, 2, 2), bool))
                    out += [(kind, pw, ph) + tuple(int(i) for i in r) for r in np.argwhere(want & ~t)]
        return out

    D_DECLARED = frozenset([(k, "sh", s) for k in "YC" for s in range(4)] +
                           [(k, what) for k in "YC" for what in ("left+inside", "right+inside", "intra", "invalid", "all_inter")] +
                           [("mixed", "Y"), ("mixed", "C")])

    def missing_d(self):
        return sorted(self.D_DECLARED - self.d, key=str)

    def missing_e(self):
        out = []
        for comp, (n_blocks, extent) in enumerate(((E_WIDTH // 16, E_WIDTH // 2), (E_HEIGHT // 16, E_HEIGHT // 2))):
            want = e_declared(n_blocks, extent)
            miss = want[~self.e[comp][want + 32768]]
            out += [("xy"[comp], int(s)) for s in miss[:20]]
            # all 16 fractions at a negative, the zero and a positive whole part
            seen = np.flatnonzero(self.e[comp]) - 32768
            for whole in (-1, 0, 1):
                sel = seen[np.sign(seen >> 4) == whole]
                out += [("xy"[comp], "fraction", whole, f) for f in range(16) if f not in set(sel & 15)]
        return out

    def missing_e_wrap(self):
        return sorted({(s, c) for s in (1, -1) for c in (0, 1)} - self.e_wrap)


def describe(pic, plane, x, y):
    """the case class of the block that holds pixel (x, y) of plane 0 / 1 / 2: for a failing comparison's message"""
    _, inter, _, planes = Coverage.planes(pic)
    P = planes[0 if plane == 0 else 1]
    mbw, _ = mb_dims(pic["w"], pic["h"])
    if plane == 0:
        mb, b = (y // 16) * mbw + x // 16, 2 * ((y % 16) // 8) + (x % 16) // 8
    else:
        mb, b = (y // 8) * mbw + x // 8, 0
    mvx, mvy = int(P["mvx"][mb, b]), int(P["mvy"][mb, b])
    return ("table (%s) %s: plane %d pixel (%d, %d): plane width %d height %d, block column %d, u = %d, ix = %d, v = %d, iy = %d, "
            "vector (%d, %d), %s macroblock %d (type %d, record vectors %s)"
            % (pic["table"], pic["tag"], plane, x, y, P["pw"], P["ph"], int(P["px"][mb, b]) // 8, int(P["px"][mb, b]) + (mvx >> 1),
               mvx & 1, int(P["py"][mb, b]) + (mvy >> 1), mvy & 1, mvx, mvy, "inter" if inter[mb] else "intra", mb,
               int(pic["mbs"][mb]["mb_type"]) if mb < len(pic["mbs"]) else 0,
               pic["mbs"][mb]["mv"].tolist() if mb < len(pic["mbs"]) else None))


def first_difference(pic, got, want):
    """None, or the description of the first differing pixel of three flat planes"""
    w, h = pic["w"], pic["h"]
    for k, (g, e, pw) in enumerate(zip(got, want, (w, (w + 1) // 2, (w + 1) // 2))):
        g, e = np.asarray(g).ravel(), np.asarray(e).ravel()
        if g.shape != e.shape:
            return "plane %d: %d bytes for %d" % (k, g.size, e.size)
        bad = np.flatnonzero(g != e)
        if bad.size:
            y, x = divmod(int(bad[0]), pw)
            return "%d bytes differ; first: got %d, expected %d at %s" % (bad.size, g[bad[0]], e[bad[0]], describe(pic, k, x, y))
    return None
