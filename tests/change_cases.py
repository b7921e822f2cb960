"""The case table of the change maps (k_change, k_change_select: h263-rs_amd/csrc/change_kernel.inl), shared by the CPU checker's
tests (test_sim_change.py) and the GPU tests (test_gpu_change.py).  The shapes are the smallest at which the kernel can still go
wrong: a wave's segment is 1024 pixels, a lane's chunk 16, a cell 8 .. 64.

A case names the picture size, the cell, the count, the two sets' placement (base offset, pitch, picture stride), the data and the
thresholds.  build(name) makes the two buffers -- exactly the sets' bytes, every byte outside the W x H rows random and different in
cur and prev, so that padding which entered a sum would show in EVERY case -- and expected(built) is the reference's answer
(change_ref).  check_hazards() asserts on the reference alone that each hazard the table is there for really occurs."""
import zlib

import numpy as np

import change_ref as ref

SEG = 1024                      # pixels of a wave's segment (CHANGE_SEG)
VALID, SET1 = 1, 2              # the per-picture words (CHANGE_VALID, CHANGE_SET1)
CASES = {}


def _case(name, w, h, cl, n=2, data="random", thr=0, min_changed=1, roll=0, cur=(0, "tight", "tight"), prev=(0, "tight", "tight"), **more):
    assert name not in CASES, name
    CASES[name] = dict(w=w, h=h, cl=cl, n=n, data=data, thr=thr, min_changed=min_changed, roll=roll, cur=cur, prev=prev, **more)


# ---- sizes: each with each cell, the placements and roll taking turns
SIZES = [(1, 1), (7, 3), (16, 16), (17, 9), (33, 65), (100, 60), (176, 144), (1023, 8), (1024, 8), (1025, 9), (1040, 8), (2049, 8)]
PLACES = [((0, "tight", "tight"), (0, "tight", "tight")), ((0, "r16", "tight"), (16, "r16", "padded16")),      # (16-byte paths)
          ((1, "plus1", "padded"), (5, "tight", "tight")), ((4, "r16", "tight"), (0, "plus1", "padded")),       # (bytes; 4-byte path)
          ((16, "r16", "padded16"), (4, "r16", "tight")), ((5, "plus1", "tight"), (1, "plus1", "padded"))]
k = 0
for (w, h) in SIZES:
    for cl in (3, 4, 5, 6):
        pc, pp = PLACES[k % len(PLACES)]
        _case("size_%dx%d_c%d" % (w, h, 1 << cl), w, h, cl, thr=85 << (2 * cl), roll=(k // 2) & 1, cur=pc, prev=pp)
        k += 1
# ---- heights c-1, c, c+1 for each cell
for cl in (3, 4, 5, 6):
    for dh in (-1, 0, 1):
        pc, pp = PLACES[k % len(PLACES)]
        _case("height_c%d%+d" % (1 << cl, dh), 40, (1 << cl) + dh, cl, thr=85 << (2 * cl), roll=k & 1, cur=pc, prev=pp)
        k += 1
# ---- base offsets 0, 1, 5, 16, chosen independently for cur and prev, the pitches taking turns
PITCHES = ["tight", "plus1", "r16"]
for i, oc in enumerate((0, 1, 5, 16)):
    for j, op in enumerate((0, 1, 5, 16)):
        _case("base_%d_%d" % (oc, op), 100, 60, 4, thr=700, roll=(i + j) & 1, cur=(oc, PITCHES[(i + j) % 3], "tight"),
              prev=(op, PITCHES[(i + 2 * j) % 3], "padded" if j & 1 else "tight"))
# ---- cur stride 0: every picture the same plane (prev differs per picture)
_case("cur_stride_0", 33, 65, 3, n=3, thr=300, cur=(0, "tight", "zero"), prev=(1, "plus1", "padded"))
_case("cur_stride_0_roll", 100, 60, 5, n=3, thr=9000, roll=1, cur=(16, "r16", "zero"), prev=(0, "r16", "padded16"))
# ---- data
_case("equal", 100, 60, 4, data="equal", cur=(1, "plus1", "padded"), prev=(0, "r16", "padded16"))
_case("equal_wide", 1030, 8, 3, data="equal", cur=(0, "r16", "tight"), prev=(0, "r16", "tight"))
_case("extreme_c64", 176, 144, 6, data="extreme", thr=0xFFFFFFFF)
_case("extreme_c64_wide", 176, 144, 6, data="extreme", thr=1044479, roll=1, cur=(0, "r16", "tight"), prev=(16, "r16", "tight"))
# one differing pixel (picture, y, x, cur value - prev value) each: the corners of cell (1, 2), the last column and row
for cl in (3, 4, 5, 6):
    c = 1 << cl
    _case("corners_c%d" % c, 3 * c + 5, 2 * c + 3, cl, data="pixels", roll=cl & 1, cur=(0, "r16", "tight"), prev=(5, "plus1", "padded"),
          pixels=[(0, c, 2 * c, 3), (0, c, 3 * c - 1, 5), (0, 2 * c - 1, 2 * c, 7), (0, 2 * c - 1, 3 * c - 1, 11), (1, 2 * c + 2, 3 * c + 4, 13),
                  (1, 0, 3 * c + 4, 17), (1, 2 * c + 2, 0, 19)],
          named={(0, 1, 2): 26, (1, 2, 3): 13, (1, 0, 3): 17, (1, 2, 0): 19})
    # ... and on both sides of a segment boundary
    _case("segment_c%d" % c, 1025, 9, cl, data="pixels", cur=(0, "r16", "tight"), prev=(0, "r16", "tight") if cl & 1 else (1, "tight", "tight"),
          pixels=[(0, 8, 1023, 200), (1, 0, 1024, -100)], named={(0, 8 >> cl, 1023 >> cl): 200, (1, 0, 1024 >> cl): 100})
_case("segment_2049", 2049, 8, 3, data="pixels", pixels=[(0, 7, 2047, 1), (0, 0, 2048, 2), (1, 3, 1024, 4), (1, 3, 1023, 8)],
      named={(0, 0, 255): 1, (0, 0, 256): 2, (1, 0, 128): 4, (1, 0, 127): 8})
# ---- thresholds, on random data: thr names a cell (picture, cy, cx) of the reference's grid and what to add to its SAD
_case("thr_0", 100, 60, 4, thr=0)
_case("thr_equal", 100, 60, 4, thr=("cell", 0, 1, 2, 0))                   # sad == threshold: not changed
_case("thr_minus_1", 100, 60, 4, thr=("cell", 0, 1, 2, -1))                # changed
_case("thr_max", 100, 60, 4, thr=0xFFFFFFFF)
# an edge cell for which the scaled and the raw comparison disagree: cell (0, 1) of 17x9 holds 1 x 9 pixels, SAD 100, threshold 200
_case("thr_edge_disagrees", 17, 9, 4, data="pixels", thr=200, pixels=[(0, 8, 16, 100), (1, 0, 0, 100)], named={(0, 0, 1): 100, (1, 0, 0): 100})
_case("thr_edge_disagrees_c64", 100, 60, 6, data="random", thr=64 * 60 * 70)         # (a mean of 70 a pixel; random data has about 85)
# ---- selection
for m, what in ((0, "0"), (1, "1"), (4, "all"), (5, "all_plus_1")):
    _case("min_changed_" + what, 16, 16, 3, n=3, data="every_third", thr=0, min_changed=m)
for n in (1, 3, 65, 130):
    _case("select_n%d" % n, 16, 16, 3, n=n, data="every_third", thr=0, min_changed=1, cur=(0, "r16", "tight"), prev=(1, "tight", "tight"))
_case("select_n130_roll", 16, 16, 4, n=130, data="every_third", thr=5, min_changed=1, roll=1)
# ---- launches of thousands of work items, in which a wave takes several (change_items_per_wave: items / 2048): 65 cell rows a
# picture, so the last wave of a picture has fewer items than the others
_case("many_items_2", 9, 515, 3, n=70, thr=85 << 6, roll=1, cur=(0, "r16", "tight"), prev=(0, "r16", "tight"))
_case("many_items_4", 9, 515, 3, n=130, thr=85 << 6, min_changed=65, cur=(1, "tight", "tight"), prev=(0, "r16", "padded16"))
# ---- per-picture words (what h263mi_batch_change_last hands the waves): an invalid picture, pictures in either frame set.  The
# plain entry point has no words: these run in the CPU checker, and on the GPU through the batch
_case("words_invalid_and_sets", 100, 60, 4, n=4, thr=500, min_changed=0, roll=1, cur=(0, "r16", "padded16"), prev=(5, "plus1", "padded"),
      words=[VALID | SET1, 0, VALID, VALID | SET1])
_case("words_all_invalid", 33, 65, 3, n=2, thr=0, min_changed=0, roll=1, words=[0, 0])

# the cases the two mutants of the CPU checker must fail (test_sim_change.py)
MUTANT_CASES = {
    "H263MI_MUTATE_CHANGE_EDGE_AS_FULL": ["thr_edge_disagrees", "thr_edge_disagrees_c64"],
    "H263MI_MUTATE_CHANGE_SEGMENT_CELL": ["segment_c8", "segment_c16", "segment_c32", "segment_c64", "segment_2049"],
}


class Built:
    pass


def _pitch(kind, w):
    return {"tight": w, "plus1": w + 1, "r16": (w + 15) // 16 * 16}[kind]


def _stride(kind, pitch, w, h):
    foot = h * pitch
    return {"tight": foot, "padded": foot + 37, "padded16": (foot + 15) // 16 * 16 + 48, "zero": 0}[kind]


def _place(spec, w, h, n, sets=1):
    """-> (base offset, pitch, stride, bytes of the buffer, bytes from set 0 to set 1)"""
    off, pk, sk = spec
    pitch = _pitch(pk, w)
    stride = _stride(sk, pitch, w, h)
    one_set = (n - 1) * stride + (h - 1) * pitch + w
    set1 = (n * stride + 15) // 16 * 16 if sets == 2 else 0
    return off, pitch, stride, off + set1 + one_set, set1


def _rows(buf, off, pitch, stride, p, w, h):
    """the W x H rows of picture p as a view of the buffer"""
    return np.lib.stride_tricks.as_strided(buf[off + p * stride:], shape=(h, w), strides=(pitch, 1))


_built = {}


def build(name):
    if name in _built:
        return _built[name]
    cs = CASES[name]
    b = Built()
    b.name, b.w, b.h, b.cl, b.n, b.roll, b.min_changed = name, cs["w"], cs["h"], cs["cl"], cs["n"], cs["roll"], cs["min_changed"]
    b.c = 1 << b.cl
    b.gw, b.gh = -(-b.w // b.c), -(-b.h // b.c)
    b.words = cs.get("words")
    b.valid = [bool(x & VALID) for x in b.words] if b.words else [True] * b.n
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    b.cur_off, b.cur_pitch, b.cur_stride, cur_bytes, b.set1 = _place(cs["cur"], b.w, b.h, b.n, 2 if b.words else 1)
    b.prev_off, b.prev_pitch, b.prev_stride, prev_bytes, _ = _place(cs["prev"], b.w, b.h, b.n)
    b.cur_buf = rng.integers(0, 256, cur_bytes, dtype=np.uint8)
    b.prev_buf = rng.integers(0, 256, prev_bytes, dtype=np.uint8)
    # where picture p's cur plane lies
    b.cur_at = [b.cur_off + (b.set1 if b.words and b.words[p] & SET1 else 0) for p in range(b.n)]
    kind = cs["data"]
    for p in range(b.n):
        cur = _rows(b.cur_buf, b.cur_at[p], b.cur_pitch, b.cur_stride, p, b.w, b.h)
        prev = _rows(b.prev_buf, b.prev_off, b.prev_pitch, b.prev_stride, p, b.w, b.h)
        if kind == "extreme":
            cur[:] = 255
            prev[:] = 0
        elif kind in ("equal", "pixels") or (kind == "every_third" and p % 3):
            prev[:] = cur
        elif kind == "every_third":
            prev[:] = cur ^ 1                    # every pixel differs by one: all cells changed at threshold 0
    for (p, y, x, d) in cs.get("pixels", []):
        cur = _rows(b.cur_buf, b.cur_at[p], b.cur_pitch, b.cur_stride, p, b.w, b.h)
        prev = _rows(b.prev_buf, b.prev_off, b.prev_pitch, b.prev_stride, p, b.w, b.h)
        v = 128 + (d + 1) // 2
        cur[y, x] = v
        prev[y, x] = v - d
    b.cur_planes = np.stack([_rows(b.cur_buf, b.cur_at[p], b.cur_pitch, b.cur_stride, p, b.w, b.h) for p in range(b.n)]).copy()
    b.prev_planes = np.stack([_rows(b.prev_buf, b.prev_off, b.prev_pitch, b.prev_stride, p, b.w, b.h) for p in range(b.n)]).copy()
    b.grid = ref.cells(b.cur_planes, b.prev_planes, b.c)
    thr = cs["thr"]
    if isinstance(thr, tuple):
        _, p, cy, cx, add = thr
        thr = int(b.grid[p, cy, cx]) + add
    b.thr = thr
    b.named = cs.get("named")
    b.cur_buf.setflags(write=False)
    b.prev_buf.setflags(write=False)
    _built[name] = b
    return b


_expected = {}


def expected(b):
    """-> (the (n, gh, gw) grid, of which only the valid pictures' cells are written; the summaries; the selected indices; prev's
    buffer after the launch)"""
    if b.name not in _expected:
        summ = ref.summaries(b.grid, b.w, b.h, b.c, b.thr, b.valid)
        sel = ref.select(summ, b.min_changed, b.valid)
        after = b.prev_buf.copy()
        if b.roll:
            for p in range(b.n):
                if b.valid[p]:
                    _rows(after, b.prev_off, b.prev_pitch, b.prev_stride, p, b.w, b.h)[:] = b.cur_planes[p]
        after.setflags(write=False)
        _expected[b.name] = (b.grid, summ, sel, after)
    return _expected[b.name]


def check_hazards():
    """On the reference alone: every hazard the table is there for occurs among its cases."""
    # sad == threshold is not changed, sad - 1 is
    b = build("thr_equal")
    assert b.thr == b.grid[0, 1, 2] > 0 and not ref.changed(b.grid[0, 1, 2], b.c, b.thr, ref.pixels(b.w, b.h, b.c, 1, 2))
    assert ref.pixels(b.w, b.h, b.c, 1, 2) == b.c * b.c
    b1 = build("thr_minus_1")
    assert b1.thr == b1.grid[0, 1, 2] - 1 and ref.changed(b1.grid[0, 1, 2], b1.c, b1.thr, b1.c * b1.c)
    assert expected(build("thr_max"))[1][0][1] == 0 and expected(build("thr_0"))[1][0][1] == b.gw * b.gh
    # an edge cell that the scaled comparison calls changed and the raw one does not
    for name, (p, cy, cx) in (("thr_edge_disagrees", (0, 0, 1)), ("thr_edge_disagrees_c64", (0, 0, 1))):
        e = build(name)
        sad, npix = int(e.grid[p, cy, cx]), ref.pixels(e.w, e.h, e.c, cy, cx)
        assert npix < e.c * e.c and ref.changed(sad, e.c, e.thr, npix) and not sad > e.thr, (name, sad, npix)
    e = build("thr_edge_disagrees")
    assert [s[1] for s in expected(e)[1]] == [1, 0]          # the same SAD in a full cell stays below the threshold
    # the largest sums: a full cell of c = 64 at 255, a picture's sum above 2^20
    x = build("extreme_c64")
    assert x.grid.max() == 64 * 64 * 255 and expected(x)[1][0][0] == 176 * 144 * 255 > 1 << 20
    assert expected(x)[1][0][1] == 0 and expected(build("extreme_c64_wide"))[1][0][1] == 9       # (the edge cells by their mean)
    # a differing pixel lands in exactly its named cell
    n_named = 0
    for name in CASES:
        c = build(name)
        if c.named:
            got = {(int(p), int(cy), int(cx)): int(c.grid[p, cy, cx]) for p, cy, cx in zip(*np.nonzero(c.grid))}
            assert got == c.named, (name, got)
            n_named += 1
    assert n_named >= 10
    # a segment crossing: differing pixels in columns 1023 and 1024
    for name in MUTANT_CASES["H263MI_MUTATE_CHANGE_SEGMENT_CELL"]:
        s = build(name)
        cols = {cx for (_, _, cx) in s.named}
        assert (SEG - 1) >> s.cl in cols and SEG >> s.cl in cols and s.w > SEG
    # padding alone differs: all sums 0
    for name in ("equal", "equal_wide"):
        q = build(name)
        assert not q.grid.any() and (q.cur_planes == q.prev_planes).all() and expected(q)[2] == []
    assert build("equal").cur_pitch > build("equal").w and build("equal_wide").cur_pitch > build("equal_wide").w
    # selections of none and of all, a list that is not contiguous and crosses a ballot word
    assert expected(build("min_changed_all_plus_1"))[2] == [] and expected(build("min_changed_0"))[2] == [0, 1, 2]
    assert expected(build("min_changed_all"))[2] == [0] == expected(build("min_changed_1"))[2]
    assert expected(build("select_n130"))[2] == list(range(0, 130, 3)) and expected(build("select_n65"))[2][-1] == 63
    assert expected(build("select_n1"))[2] == [0]
    # an invalid picture is never selected, even at min_changed_cells 0
    assert expected(build("words_invalid_and_sets"))[2] == [0, 2, 3] and expected(build("words_all_invalid"))[2] == []
    # launches in which a wave takes 2 and 4 items, 65 a picture
    for name, k in (("many_items_2", 2), ("many_items_4", 4)):
        m = build(name)
        assert m.gh == 65 and m.w <= SEG and (m.n * m.gh) // 2048 == k
    assert 0 < len(expected(build("many_items_4"))[2]) < 130
    # every access path occurs: both sets on 16-byte accesses, on 4-byte ones, on bytes; a short chunk at the right edge
    paths = set()
    for name in CASES:
        c = build(name)
        for off, pitch, stride in ((c.cur_off, c.cur_pitch, c.cur_stride), (c.prev_off, c.prev_pitch, c.prev_stride)):
            m = off | pitch | stride
            paths.add(16 if m % 16 == 0 else 4 if m % 4 == 0 else 1)
    assert paths == {16, 4, 1}
    assert any(CASES[n]["w"] % 16 for n in CASES) and any(CASES[n]["w"] % 16 == 0 for n in CASES)
