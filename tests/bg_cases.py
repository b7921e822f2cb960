"""The case table of the background model (k_bg_begin, k_bg: h263-rs_amd/csrc/background_kernel.inl), shared by the CPU checker's tests
(test_sim_bg.py) and the GPU tests (test_gpu_bg.py).  The shapes are the smallest at which the kernel can still go wrong: a wave's
segment is 1024 pixels, a lane's chunk 16, a cell 8 .. 64.

A case is a sequence of 1 .. 6 calls on ONE state: the picture size, the cell, the count, the placement of cur and of the mask (base
offset, pitch, picture stride: change_cases.PLACES), the parameters, the state in front of the first call (all zero, or preloaded
words and heads) and per call the pictures, the cut list and the per-picture words.  build(name) makes the buffers -- cur of exactly
the set's bytes, every byte outside the W x H rows random -- and expected(built) is the reference's answer after every call (bg_ref).
check_hazards() asserts on the reference alone that each hazard the table is there for really occurs; convergence() and
stopped_object() are the two scenarios, asserted on the reference too."""
import zlib

import numpy as np

import bg_ref as ref
import change_cases as cc
import change_ref

SEG = 1024                      # pixels of a wave's segment (CHANGE_SEG)
VALID, SET1 = 1, 2              # the per-picture words (CHANGE_VALID, CHANGE_SET1)
SENTINEL = 0xC3C3C3C3
CASES = {}
TIGHT = (0, "tight", "tight")
WIDE = (0, "r16", "tight")


def _case(name, w, h, cl, calls, n=2, cur=TIGHT, mask=None, state=None, **prm):
    assert name not in CASES and (isinstance(calls, str) or 1 <= len(calls) <= 6), name
    CASES[name] = dict(w=w, h=h, cl=cl, n=n, calls=calls, cur=cur, mask=mask, state=state, prm=prm)


def _call(data, cut=None, cut_count=None, cut_extra=(), words=None, **args):
    """cut: the listed pictures; cut_count: the count word (None: len(cut)); cut_extra: entries behind the n that a call may read"""
    return dict(data=data, cut=cut, cut_count=cut_count, cut_extra=list(cut_extra), words=words, args=args)


# ---- the pictures of a call: f(b, last planes or None, rng, **args) -> (n, h, w) uint8
def _random(b, last, rng):
    return rng.integers(0, 256, (b.n, b.h, b.w), dtype=np.uint8)


def _drift(b, last, rng, noise=6):
    """every pixel moves a little, a rectangle of every picture a lot"""
    out = np.clip(last.astype(np.int64) + rng.integers(-noise, noise + 1, last.shape), 0, 255).astype(np.uint8)
    for p in range(b.n):
        y0, x0 = int(rng.integers(0, b.h)), int(rng.integers(0, b.w))
        y1, x1 = min(b.h, y0 + max(1, b.h // 2)), min(b.w, x0 + max(1, b.w // 3))
        out[p, y0:y1, x0:x1] = 255 - last[p, y0:y1, x0:x1]
    return out


def _const(b, last, rng, value=0):
    return np.full((b.n, b.h, b.w), value, np.uint8)


def _pixels(b, last, rng, base=128, pixels=()):
    out = np.full((b.n, b.h, b.w), base, np.uint8)
    for (p, y, x, v) in pixels:
        out[p, y, x] = v
    return out


def _halves(b, last, rng, left=255, right=0):
    out = np.full((b.n, b.h, b.w), right, np.uint8)
    out[:, :, :b.w // 2] = left
    return out


def _every_third(b, last, rng):
    out = last.copy()
    out[::3] = last[::3] ^ 0x80                                       # every pixel of pictures 0, 3, 6 ... moves by 128
    return out


def _block(b, last, rng, base=None, at=None, size=16, value=200):
    out = base.copy()
    if at is not None:
        out[:, at[0]:at[0] + size, at[1]:at[1] + size] = value
    return out


# ---- the state in front of the first call: f(b, state, rng) fills the zeroed buffer
def _preload(age=5, word=None, words=None, ages=None):
    def fill(b, state, rng):
        for p in range(b.n):
            ref.head_of(state, p, b.w, b.h)[0] = ages[p] if ages else age
            v = ref.words_of(state, p, b.w, b.h)
            if words is not None:
                v[:, :b.w] = words(b, p, rng)
            else:
                v[:, :b.w] = word
    return fill


# ---- sizes: each with each cell; the placements, the shifts and the threshold taking turns
SIZES = cc.SIZES
FG_SHIFTS = [ref.KEEP, 0, 1, 2, 3, 4, 5, 6, 7]
k = 0
for (w, h) in SIZES:
    for cl in (3, 4, 5, 6):
        pc, pm = cc.PLACES[k % len(cc.PLACES)]
        _case("size_%dx%d_c%d" % (w, h, 1 << cl), w, h, cl, [_call(_random), _call(_drift), _call(_drift)], cur=pc, mask=pm if k % 5 else None,
              learn=k % 8, fg_learn=FG_SHIFTS[k % 9], pix_thr=(0, 10, 24, 40)[k % 4], cell_thr=(1 << (2 * cl)) // 8, min_changed=1)
        k += 1
# ---- heights c-1, c, c+1 for each cell (an item's rows: odd, even, one)
for cl in (3, 4, 5, 6):
    for dh in (-1, 0, 1):
        pc, pm = cc.PLACES[k % len(cc.PLACES)]
        _case("height_c%d%+d" % (1 << cl, dh), 40, (1 << cl) + dh, cl, [_call(_random), _call(_drift)], cur=pc, mask=pm, learn=k % 8,
              fg_learn=FG_SHIFTS[k % 9], pix_thr=12, cell_thr=(1 << (2 * cl)) // 16)
        k += 1
# ---- the verdict: |c - r| equal to the threshold and one above it, on both sides
_case("thr_equal_and_above", 40, 20, 3, [_call(_pixels, base=100, pixels=[(0, 3, 5, 124), (0, 3, 6, 125), (0, 10, 20, 76), (0, 10, 21, 75)])],
      n=1, state=_preload(word=100 << 7), learn=2, fg_learn=ref.KEEP, pix_thr=24, cur=WIDE, mask=WIDE)
# a word whose fraction is exactly 64 rounds up (r = 101), one of 63 down (r = 100): the rounding decides the verdict
_case("rounding_fraction_64", 40, 20, 3,
      [_call(_pixels, base=101, pixels=[(0, 2, 2, 125), (0, 2, 3, 76), (0, 2, 4, 126), (1, 4, 4, 124), (1, 4, 5, 76), (1, 4, 6, 75)])],
      n=2, state=_preload(words=lambda b, p, rng: (100 << 7) + 64 - p), learn=7, fg_learn=ref.KEEP, pix_thr=24, mask=TIGHT)
# ---- the step: 0 < |d| < 2^s on both sides moves by one, arrives, and stays
_case("small_d_both_signs", 40, 20, 3, [_call(_const, value=100)] * 4, n=2,
      state=_preload(words=lambda b, p, rng: (100 << 7) + (3 if p else -3)), learn=4, fg_learn=4, pix_thr=255)
# d = +-32640 at shift 0 and 7, as background and as foreground
for name, learn, fg_learn, thr in (("extreme_d_s0", 0, 7, 255), ("extreme_d_s7", 7, 0, 255), ("extreme_d_fg_s0", 7, 0, 10),
                                    ("extreme_d_fg_s7", 0, 7, 10)):
    _case(name, 48, 9, 4, [_call(_halves), _call(_halves)], n=1, state=_preload(words=lambda b, p, rng: np.where(np.arange(b.w) < b.w // 2, 0, 32640)),
          learn=learn, fg_learn=fg_learn, pix_thr=thr, cur=WIDE, mask=(16, "r16", "padded16"))
# a foreground pixel keeps its word / learns at another rate than the background
for name, fg_learn in (("fg_keeps_its_word", ref.KEEP), ("fg_shift_differs", 6)):
    _case(name, 40, 20, 3, [_call(_pixels, base=52, pixels=[(0, y, x, 200) for y in range(4, 12) for x in range(8, 24)])] * 2, n=1,
          state=_preload(word=50 << 7), learn=2, fg_learn=fg_learn, pix_thr=24, cell_thr=32, mask=(5, "plus1", "padded"))
# ---- cells: an edge cell for which the scaled and the raw comparison disagree (cell (0, 1) of 17 x 9 holds 1 x 9 pixels)
_case("thr_edge_disagrees", 17, 9, 4, [_call(_pixels, base=0, pixels=[(0, y, 16, 200) for y in range(5)] + [(1, y, 0, 200) for y in range(5)])],
      state=_preload(word=0), pix_thr=24, cell_thr=100)
# a foreground pixel on each side of a segment boundary
for cl in (3, 4, 5, 6):
    _case("segment_c%d" % (1 << cl), 1025, 9, cl, [_call(_pixels, base=128, pixels=[(0, 8, 1023, 255), (1, 0, 1024, 0)])],
          state=_preload(word=128 << 7), pix_thr=24, cur=WIDE if cl & 1 else (1, "tight", "tight"), mask=WIDE if cl & 2 else None,
          named={(0, 8 >> cl, 1023 >> cl): 1, (1, 0, 1024 >> cl): 1})
_case("segment_2049", 2049, 8, 3, [_call(_pixels, base=128, pixels=[(0, 7, 2047, 0), (0, 0, 2048, 255), (1, 3, 1024, 0), (1, 3, 1023, 255)])],
      state=_preload(word=128 << 7), pix_thr=24, cur=WIDE, named={(0, 0, 255): 1, (0, 0, 256): 1, (1, 0, 128): 1, (1, 0, 127): 1})
# c = 8: the two cells of one chunk
_case("two_cells_per_chunk", 40, 8, 3, [_call(_pixels, base=128, pixels=[(0, 1, 19, 0), (0, 2, 27, 0), (0, 3, 28, 0), (1, 7, 23, 255), (1, 0, 24, 255)])],
      state=_preload(word=128 << 7), pix_thr=24, cur=WIDE, named={(0, 0, 2): 1, (0, 0, 3): 2, (1, 0, 2): 1, (1, 0, 3): 1})
# ---- the mode: an initialisation by a cut; entries >= n are ignored; a count above n is clamped to n entries
_case("init_by_cut", 33, 17, 3, [_call(_random), _call(_drift), _call(_drift, cut=[2, 7, 0])], n=4, learn=3, fg_learn=5, pix_thr=10, cell_thr=8,
      mask=(1, "plus1", "padded"))
_case("cut_count_clamped", 33, 17, 3, [_call(_random), _call(_drift, cut=[1, 9, 9], cut_count=8, cut_extra=[0, 2, 0, 2, 0])], n=3, learn=3,
      fg_learn=5, pix_thr=10, cell_thr=8)
# warm-up: ages 1 and 2 = warmup - 1 learn without a verdict, age 3 = warmup judges
_case("warmup_3", 40, 20, 3, [_call(_random)] + [_call(_drift)] * 4, warmup=3, learn=1, fg_learn=ref.KEEP, pix_thr=20, cell_thr=4, mask=WIDE, cur=WIDE)
# the age saturates
_case("age_saturates", 16, 16, 3, [_call(_drift), _call(_drift)], state=_preload(ages=[0xFFFFFFFE, 0xFFFFFFFF], words=lambda b, p, rng: 77 << 7),
      learn=2, pix_thr=20, start=77)
# ---- selection
for m, what in ((0, "0"), (1, "1"), (4, "all"), (5, "all_plus_1")):
    _case("min_changed_" + what, 16, 16, 3, [_call(_random), _call(_every_third)], n=3, pix_thr=24, cell_thr=0, min_changed=m)
for n in (1, 3, 65, 130):
    _case("select_n%d" % n, 16, 16, 3, [_call(_random), _call(_every_third)], n=n, pix_thr=24, cur=WIDE)
# ---- launches of thousands of work items, in which a wave takes several (change_items_per_wave: items / 2048): 65 cell rows a
# picture, so the last wave of a picture has fewer items than the others
_case("many_items_2", 9, 515, 3, [_call(_random), _call(_drift)], n=70, learn=2, fg_learn=4, pix_thr=16, cell_thr=8, cur=WIDE, mask=WIDE)
_case("many_items_4", 9, 515, 3, [_call(_random), _call(_drift)], n=130, learn=3, pix_thr=16, cell_thr=8, min_changed=20, cur=(1, "tight", "tight"))
# ---- per-picture words (what h263mi_batch_background_last hands the waves): an invalid picture, pictures in either frame set.
# The plain entry point has no words: these run in the CPU checker, and on the GPU through the batch
_case("words_invalid_and_sets", 100, 60, 4, [_call(_random, words=[VALID | SET1, 0, VALID, VALID | SET1]),
                                             _call(_drift, words=[VALID, 0, VALID | SET1, VALID | SET1]),
                                             _call(_drift, words=[VALID | SET1, VALID, 0, VALID])],
      n=4, learn=2, fg_learn=5, pix_thr=12, cell_thr=20, min_changed=0, cur=(0, "r16", "padded16"), mask=(5, "plus1", "padded"))
_case("words_all_invalid", 33, 65, 3, [_call(_random, words=[0, 0])], min_changed=0, mask=TIGHT)
# ---- the scenarios' last calls (convergence(), stopped_object() below hold the whole of them)
_case("converge_arrival", 40, 20, 3, [_call(_const, value=255)] * 6, n=1, state="convergence", learn=3, fg_learn=3, pix_thr=255)
_case("stopped_object", 64, 48, 3, "stopped_object", n=1, learn=4, fg_learn=6, pix_thr=24, cell_thr=16, cur=WIDE, mask=WIDE)

# the cases the two mutants of the CPU checker must fail (test_sim_bg.py); they pass every case that affected() does not name
MUTANT_CASES = {
    "H263MI_MUTATE_BG_STEP_FLOOR": ["small_d_both_signs", "converge_arrival"],
    "H263MI_MUTATE_BG_JUDGE_AFTER": ["thr_equal_and_above", "rounding_fraction_64"],
}


class Built:
    pass


class Call:
    pass


def convergence(shift=3, start=0, value=255):
    """A constant plane from a far state: -> (the word before every call, the last entry the word that stays)"""
    b, seen = np.array([start], np.int64), []
    c = np.array([value], np.int64)
    while True:
        seen.append(int(b[0]))
        nxt = ref.moved(c, b, shift)
        if nxt[0] == b[0]:
            return seen
        b = nxt


def stopped_object_pictures(w=64, h=48, still=2, seed=11):
    """a textured background; a 16 x 16 block enters, moves for three pictures, then stands still"""
    base = np.random.default_rng(seed).integers(50, 70, (1, h, w), dtype=np.uint8)
    class G:
        n = 1
    g = G()
    pics = [base.copy()]
    for x in (8, 16, 24):
        pics.append(_block(g, None, None, base=base, at=(16, x)))
    pics += [pics[-1].copy() for _ in range(still)]
    return pics


def stopped_object(prm, still):
    """-> per picture (changed cells of the change map with roll = 1, changed cells of the background model, the background
    model's changed cells inside the block's cells)"""
    pics = stopped_object_pictures(still=still)
    n, h, w = pics[0].shape
    state, prev, out = ref.empty_state(n, w, h), pics[0], []
    for pic in pics:
        grid = change_ref.cells(pic, prev, prm.c)
        moved = change_ref.summaries(grid, w, h, prm.c, prm.cell_thr * 8)[0][1]      # (a SAD threshold of 8 a foreground pixel)
        prev = pic
        _, grid, summ, _ = ref.call(state, pic, prm)
        inside = sum(change_ref.changed(grid[0, cy, cx], prm.c, prm.cell_thr, prm.c * prm.c) for cy in (2, 3) for cx in (3, 4))
        out.append((moved, summ[0][1], inside))
    return out


def stopped_object_k(prm, cap=400):
    """the still pictures for which the block's four cells all stay changed, with the case's shifts (cap: it never leaves)"""
    rows = stopped_object(prm, cap)
    k = 0
    while k < cap and rows[4 + k][2] == 4:
        k += 1
    return k


def _align(m):
    return 16 if m % 16 == 0 else 4 if m % 4 == 0 else 1


_built = {}


def build(name):
    if name in _built:
        return _built[name]
    cs = CASES[name]
    b = Built()
    b.name, b.w, b.h, b.cl, b.n = name, cs["w"], cs["h"], cs["cl"], cs["n"]
    prm = dict(cs["prm"])
    b.named = prm.pop("named", None)
    start = prm.pop("start", None)
    b.prm = ref.Params(b.cl, **prm)
    b.c = b.prm.c
    b.gw, b.gh = -(-b.w // b.c), -(-b.h // b.c)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    specs = cs["calls"]
    if specs == "stopped_object":
        pics = stopped_object_pictures(b.w, b.h)
        specs = [_call(lambda b, last, rng, pic=pic: pic) for pic in pics]
    sets = 2 if any(s["words"] for s in specs) else 1
    b.cur_off, b.cur_pitch, b.cur_stride, cur_bytes, b.set1 = cc._place(cs["cur"], b.w, b.h, b.n, sets)
    b.mask = cs["mask"] is not None
    if b.mask:
        b.mask_off, b.mask_pitch, b.mask_stride, mask_bytes, _ = cc._place(cs["mask"], b.w, b.h, b.n)
        b.mask0 = rng.integers(0, 256, mask_bytes, dtype=np.uint8)
        b.mask0.setflags(write=False)
    b.stride = ref.state_stride(b.w, b.h)
    b.state0 = ref.empty_state(b.n, b.w, b.h)
    if cs["state"] == "convergence":
        seen = convergence(b.prm.learn)
        _preload(word=seen[-6])(b, b.state0, rng)                     # five calls in front of the arrival
    elif cs["state"]:
        cs["state"](b, b.state0, rng)
    b.state0.setflags(write=False)
    b.calls, last = [], None if start is None else np.full((b.n, b.h, b.w), start, np.uint8)
    for s in specs:
        q = Call()
        q.planes = s["data"](b, last, rng, **s["args"])
        last = q.planes
        q.words = s["words"]
        q.valid = [bool(x & VALID) for x in q.words] if q.words else [True] * b.n
        q.cur_buf = rng.integers(0, 256, cur_bytes, dtype=np.uint8)
        for p in range(b.n):
            at = b.cur_off + (b.set1 if q.words and q.words[p] & SET1 else 0)
            cc._rows(q.cur_buf, at, b.cur_pitch, b.cur_stride, p, b.w, b.h)[:] = q.planes[p]
        q.cur_buf.setflags(write=False)
        q.cut = None if s["cut"] is None else np.asarray(s["cut"], np.uint32)
        q.cut_count = 0 if q.cut is None else (len(s["cut"]) if s["cut_count"] is None else s["cut_count"])
        q.cut_extra = np.asarray(s["cut_extra"], np.uint32)
        b.calls.append(q)
    _built[name] = b
    return b


_expected = {}


def expected(b, mutant=None):
    """-> per call (state after, mask buffer after or None, the (n, gh, gw) grid with SENTINEL where none is written, summaries,
    selected indices, the heads' modes)"""
    key = (b.name, mutant)
    if key not in _expected:
        state = b.state0.copy()
        mask = b.mask0.copy() if b.mask else None
        out = []
        for q in b.calls:
            fg, grid, summ, sel = ref.call(state, q.planes, b.prm, q.valid, q.cut, q.cut_count, mutant=mutant)
            if b.mask:
                for p in range(b.n):
                    if q.valid[p]:
                        cc._rows(mask, b.mask_off, b.mask_pitch, b.mask_stride, p, b.w, b.h)[:] = np.where(fg[p], 255, 0)
            cells = np.where(np.asarray(q.valid)[:, None, None], grid, SENTINEL)
            modes = [int(ref.head_of(state, p, b.w, b.h)[1]) for p in range(b.n)]
            out.append((state.copy(), mask.copy() if b.mask else None, cells, summ, sel, modes))
        _expected[key] = out
    return _expected[key]


def affected(b, mutant):
    """does the mutant's arithmetic change anything this case delivers?"""
    for good, bad in zip(expected(b), expected(b, mutant)):
        if not ((good[0] == bad[0]).all() and (good[2] == bad[2]).all() and good[3] == bad[3] and good[4] == bad[4]):
            return True
    return False


def check_hazards():
    """On the reference alone: every hazard the table is there for occurs among its cases."""
    def fg_of(name, k=0):
        b = build(name)
        st = (b.state0 if k == 0 else expected(b)[k - 1][0]).copy()
        q = b.calls[k]
        return b, ref.call(st, q.planes, b.prm, q.valid, q.cut, q.cut_count)[0]
    # |c - r| == threshold is background, one above is foreground, on both sides
    b, fg = fg_of("thr_equal_and_above")
    assert {tuple(int(v) for v in i) for i in np.argwhere(fg)} == {(0, 3, 6), (0, 10, 21)} and b.prm.pix_thr == 24
    # a fraction of exactly 64 rounds up: c = 125 against r = 101 is background (against 100 it would not be), 76 is foreground;
    # a fraction of 63 rounds down: 124 and 76 against r = 100 are background, 75 is foreground
    b, fg = fg_of("rounding_fraction_64")
    assert {tuple(int(v) for v in i) for i in np.argwhere(fg)} == {(0, 2, 3), (0, 2, 4), (1, 4, 6)}
    assert int(ref.words_of(b.state0, 0, b.w, b.h)[0, 0]) & 127 == 64 and int(ref.words_of(b.state0, 1, b.w, b.h)[0, 0]) & 127 == 63
    # 0 < |d| < 2^s on both sides: one a call, arrives exactly, stays
    b = build("small_d_both_signs")
    seq = [[int(ref.words_of(e[0], p, b.w, b.h)[0, 0]) - (100 << 7) for e in expected(b)] for p in range(2)]
    assert seq == [[-2, -1, 0, 0], [2, 1, 0, 0]] and b.prm.learn == 4
    # d = +-32640 at shifts 0 and 7, as background and as foreground
    for name, after in (("extreme_d_s0", (32640, 0)), ("extreme_d_s7", (255, 32640 - 255)), ("extreme_d_fg_s0", (32640, 0)),
                        ("extreme_d_fg_s7", (255, 32640 - 255))):
        b = build(name)
        e = expected(b)[0]
        v = ref.words_of(e[0], 0, b.w, b.h)
        assert (int(v[0, 0]), int(v[0, b.w - 1])) == after, name
        assert e[3][0][0] == (b.w * b.h if "fg" in name else 0)
    # a foreground pixel keeps its word; with another shift it learns at another rate than the background
    b = build("fg_keeps_its_word")
    v = ref.words_of(expected(b)[1][0], 0, b.w, b.h)
    assert int(v[5, 10]) == 50 << 7 and int(v[0, 0]) > 50 << 7 and expected(b)[1][3][0][0] == 8 * 16
    b = build("fg_shift_differs")
    v = ref.words_of(expected(b)[0][0], 0, b.w, b.h)
    assert int(v[5, 10]) == (50 << 7) + ((150 << 7) >> 6) and int(v[0, 0]) == (50 << 7) + ((2 << 7) >> 2) and b.prm.fg_learn != b.prm.learn
    # an edge cell that the scaled comparison calls changed and the raw one does not
    b = build("thr_edge_disagrees")
    e = expected(b)[0]
    count, npix = int(e[2][0, 0, 1]), change_ref.pixels(b.w, b.h, b.c, 0, 1)
    assert npix == 9 and count == 5 and change_ref.changed(count, b.c, b.prm.cell_thr, npix) and not count > b.prm.cell_thr
    assert [s[1] for s in e[3]] == [1, 0]                           # the same count in a full cell stays below
    # a foreground pixel lands in exactly its named cell: both sides of a segment boundary, both cells of a chunk
    named = 0
    for name in CASES:
        b = build(name)
        if b.named:
            grid = expected(b)[0][2]
            assert {(int(p), int(cy), int(cx)): int(grid[p, cy, cx]) for p, cy, cx in zip(*np.nonzero(grid))} == b.named, name
            named += 1
    assert named == 6
    for cl in (3, 4, 5, 6):
        cols = {cx for (_, _, cx) in build("segment_c%d" % (1 << cl)).named}
        assert (SEG - 1) >> cl in cols and SEG >> cl in cols
    assert {cx for (_, _, cx) in build("two_cells_per_chunk").named} == {2, 3} and build("two_cells_per_chunk").c == 8
    # INIT by age 0: the first call of a zero state, everywhere: mode, age, no foreground
    b = build("size_100x60_c16")
    e = expected(b)
    assert e[0][5] == [ref.VALID | ref.INIT] * 2 and e[0][3] == [(0, 0, 0)] * 2 and e[1][5] == [ref.VALID] * 2 and e[1][3][0][0] > 0
    assert int(ref.head_of(e[0][0], 0, b.w, b.h)[0]) == 1 and int(ref.head_of(e[2][0], 1, b.w, b.h)[0]) == 3
    # INIT by cut: pictures 0 and 2; the entry 7 >= n names nobody
    b = build("init_by_cut")
    e = expected(b)[2]
    assert e[5] == [ref.VALID | ref.INIT, ref.VALID, ref.VALID | ref.INIT, ref.VALID] and e[3][0] == (0, 0, 0) and e[3][1][0] > 0
    assert [int(ref.head_of(e[0], p, b.w, b.h)[0]) for p in range(4)] == [1, 3, 1, 3]
    # a count above n is clamped: only picture 1 is cut, though entries 3 .. 7 (which a GPU test provides) name 0 and 2
    b = build("cut_count_clamped")
    assert b.calls[1].cut_count > b.n and expected(b)[1][5] == [ref.VALID, ref.VALID | ref.INIT, ref.VALID]
    assert set(b.calls[1].cut_extra.tolist()) == {0, 2}
    # warm-up: the call at age warmup - 1 learns without a verdict, the one at age warmup judges
    b = build("warmup_3")
    e = expected(b)
    assert [x[5][0] for x in e] == [ref.VALID | ref.INIT, ref.VALID | ref.WARM, ref.VALID | ref.WARM, ref.VALID, ref.VALID]
    assert [x[3][0][0] > 0 for x in e] == [False, False, False, True, True]
    assert not (e[2][0] == e[1][0]).all()                           # (a warm call learns)
    # the age saturates
    b = build("age_saturates")
    assert [[int(ref.head_of(x[0], p, b.w, b.h)[0]) for p in range(2)] for x in expected(b)] == [[0xFFFFFFFF] * 2] * 2
    # an invalid picture: its state is untouched, its summary zero, never selected; both frame sets occur
    b = build("words_invalid_and_sets")
    e = expected(b)
    at = slice(b.stride, 2 * b.stride)
    assert (e[0][0][at] == 0).all() and (e[1][0][at] == 0).all() and e[2][5][1] == ref.VALID | ref.INIT
    assert e[1][4] == [0, 2, 3] and e[1][3][1] == (0, 0, 0) and e[2][4] == [0, 1, 3]
    assert {x & SET1 for q in b.calls for x in q.words if x & VALID} == {0, SET1}
    assert expected(build("words_all_invalid"))[0][4] == []
    # selections of none and of all, a list that is not contiguous and crosses a ballot word
    assert expected(build("min_changed_all_plus_1"))[1][4] == [] and expected(build("min_changed_0"))[1][4] == [0, 1, 2]
    assert expected(build("min_changed_all"))[1][4] == [0] == expected(build("min_changed_1"))[1][4]
    assert expected(build("select_n130"))[1][4] == list(range(0, 130, 3)) and expected(build("select_n65"))[1][4][-1] == 63
    # launches in which a wave takes 2 and 4 items, 65 a picture
    for name, k in (("many_items_2", 2), ("many_items_4", 4)):
        m = build(name)
        assert m.gh == 65 and m.w <= SEG and (m.n * m.gh) // 2048 == k
    assert 0 < len(expected(build("many_items_4"))[1][4]) < 130
    # padding words stay 0 while cur's bytes behind column W are random; every access path of cur and of the mask occurs
    paths, padded = {"cur": set(), "mask": set()}, 0
    for name in CASES:
        b = build(name)
        pw = ref.padded_width(b.w)
        if pw > b.w:
            for e in expected(b):
                for p in range(b.n):
                    assert not ref.words_of(e[0], p, b.w, b.h)[:, b.w:].any(), name
            padded += 1
        paths["cur"].add(_align(b.cur_off | b.cur_pitch | b.cur_stride))
        if b.mask:
            paths["mask"].add(_align(b.mask_off | b.mask_pitch | b.mask_stride))
    assert padded >= 20 and paths == {"cur": {16, 4, 1}, "mask": {16, 4, 1}}
    assert any(not build(n).mask for n in CASES)
    # every shift occurs as learn_shift and as fg_learn_shift
    assert {build(n).prm.learn for n in CASES} == set(range(8)) and {build(n).prm.fg_learn for n in CASES} == set(range(8)) | {ref.KEEP}
    # the mutants' named cases are affected, and enough others are not
    for mutant, names in MUTANT_CASES.items():
        assert all(affected(build(n), mutant) for n in names), mutant
        assert sum(not affected(build(n), mutant) for n in CASES) >= 8, mutant
    # ---- the scenarios
    # convergence: from 0 to 255 << 7 at shift 3, arrives exactly and stays; the case runs the last five calls and one more
    seen = convergence(3)
    assert seen[0] == 0 and seen[-1] == 255 << 7 and len(seen) > 40 and all(x < y for x, y in zip(seen, seen[1:]))
    b = build("converge_arrival")
    got = [int(ref.words_of(e[0], 0, b.w, b.h)[3, 3]) for e in expected(b)]
    assert got == seen[-5:] + [255 << 7] and got[-3] != 255 << 7
    # stopped object: the change map loses the block from the second still picture on, the background model keeps its cells
    # for all k still pictures, k the reference's own figure for the case's shifts (then the block has become background)
    prm = build("stopped_object").prm
    k = stopped_object_k(prm)
    rows = stopped_object(prm, k + 1)
    assert 50 < k < 400 and rows[0] == (0, 0, 0) and all(r[0] > 0 and r[1] > 0 for r in rows[1:4])
    assert all(r[0] == 0 for r in rows[4:])                         # (still pictures are identical: the change map is empty)
    assert all(r[2] == 4 for r in rows[4:4 + k]) and rows[4 + k][2] < 4
    e = expected(build("stopped_object"))
    assert [x[3][0][1] for x in e] == [r[1] for r in rows[:6]]
