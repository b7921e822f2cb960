"""The case table of the plane histograms (k_hist, k_hist_final, k_hist_select: h263-rs_amd/csrc/hist_kernel.inl), shared by the CPU
checker's tests (test_sim_hist.py) and the GPU tests (test_gpu_hist.py).  The shapes are the smallest at which the kernels can
still go wrong: a wave's segment is 1024 pixels, a lane's chunk 16, a work item 8 rows.

A case names the picture size, the count, the set's placement (base offset, pitch, picture stride), the data, prev, the
percentiles and the cut.  build(name) makes the buffer -- exactly the set's bytes, every byte outside the W x H rows random, so
that padding which entered a count would show in EVERY case -- and expected(built) is the reference's answer (hist_ref).
check_hazards() asserts on the reference alone that each hazard the table is there for really occurs."""
import zlib

import numpy as np

import hist_ref as ref

SEG, ROWS = 1024, 8             # pixels of a wave's segment, rows of a work item (HIST_SEG, HIST_ROWS)
VALID, SET1 = 1, 2              # the per-picture words (HIST_VALID, HIST_SET1)
SENTINEL = 0xC3C3C3C3
CASES = {}


def _case(name, w, h, n=2, data="random", place=(0, "tight", "tight"), prev="random", lo=10, hi=990, cut=500, roll=0, **more):
    assert name not in CASES, name
    CASES[name] = dict(w=w, h=h, n=n, data=data, place=place, prev=prev, lo=lo, hi=hi, cut=cut, roll=roll, **more)


# ---- sizes: every width with every height, the placements, prev and roll taking turns.  Base offsets and pitches 0, 1, 4 and 16
# from a multiple of 16: the 16-byte path, bytes, words, the 16-byte path again
WIDTHS = [1, 15, 16, 17, 63, 1023, 1024, 1025, 2049]
HEIGHTS = [1, 2, 9, 17]
PLACES = [(0, "r16", "padded16"), (1, "plus1", "padded"), (4, "r4", "padded4"), (16, "r16", "tight16"), (0, "tight", "tight"),
          (5, "tight", "tight")]
PREVS = ["random", None, "zero", "own"]
k = 0
for w in WIDTHS:
    for h in HEIGHTS:
        _case("size_%dx%d" % (w, h), w, h, place=PLACES[k % len(PLACES)], prev=PREVS[k % len(PREVS)], roll=(k // 4) & 1 if PREVS[k % len(PREVS)] else 0,
              cut=(0, 300, 500, 1000)[(k // 3) % 4])
        k += 1
# ---- each placement with a width that the edge cuts and one that it does not, at a height with a short last band
for i, pl in enumerate(PLACES):
    for w in (100, 96):
        _case("place_%d_%s_%s_w%d" % (pl + (w,)), w, 11, n=3, place=pl, prev=PREVS[i % len(PREVS)])
# ---- picture stride 0 (every picture the same plane) and pictures that overlap
_case("stride_0", 33, 20, n=3, place=(0, "r16", "zero"))
_case("stride_0_bytes", 33, 20, n=3, place=(1, "plus1", "zero"), prev=None)
_case("overlap_rows", 40, 20, n=4, place=(0, "r16", "rows2"), prev="zero", roll=1)
_case("overlap_1", 40, 20, n=4, place=(0, "tight", "one"), prev="own")
# ---- content
for v in (0, 255, 77):
    _case("flat_%d" % v, 100, 60, data=("flat", v), place=(0, "r16", "padded16"), prev="zero", roll=1, lo=0, hi=1000)
    _case("flat_%d_bytes" % v, 100, 60, data=("flat", v), place=(1, "plus1", "padded"), prev=None)
_case("alt_pixel", 100, 20, data=("alt", "pixel", 3, 250), place=(0, "r16", "tight16"))
_case("alt_16", 100, 20, data=("alt", "16", 0, 255), place=(0, "r16", "tight16"), prev="own")
_case("alt_row", 100, 21, data=("alt", "row", 128, 129), place=(4, "r4", "padded4"), prev=None)
_case("ramp", 64, 16, data="ramp", n=3, lo=500, hi=500)                    # every value exactly four times
_case("ramp_wide", 1280, 2, data="ramp", n=1, place=(0, "r16", "tight16"), prev="zero", lo=0, hi=0)
_case("decoded", 176, 144, data="decoded", n=2, place=(0, "pitch256", "padded16"), prev="zero", roll=1, lo=20, hi=980)
_case("decoded_bytes", 176, 144, data="decoded", n=2, place=(3, "plus1", "padded"), prev="random", lo=500, hi=999)
# one bin reaches 2^21 through the additions of 256 waves
_case("flat_2048x1024", 2048, 1024, n=1, data=("flat", 200), place=(0, "tight", "tight"), prev="zero", lo=1, hi=999)
# ---- the cut: 100 x 60 = 6000 pixels, cut_permille 250 -> a cut above a distance of 3000.  prev = the picture's own histogram
# with `add` more in bin 7
_case("cut_equal_and_above", 100, 60, n=4, prev=("own_plus", [3000, 3001, 2999, 0]), cut=250)
_case("cut_0", 100, 60, n=3, prev=("own_plus", [0, 1, 0]), cut=0)            # any distance at all is a cut
_case("cut_1000", 100, 60, n=3, prev=("own_plus", [12000, 12001, 1 << 31]), cut=1000)
_case("cut_first_call", 100, 60, n=2, prev="zero", cut=499, roll=1)          # a zeroed prev: distance P, a cut below 500
_case("cut_first_call_500", 100, 60, n=2, prev="zero", cut=500, roll=1)
# ---- percentiles: 600 pixels of 10, 2400 of 20, 3000 of 200 -- C(10) * 1000 == 100 * P and C(20) * 1000 == 500 * P
COUNTS = [(10, 600), (20, 2400), (200, 3000)]
_case("pctl_exact", 100, 60, data=("counts", COUNTS), lo=100, hi=500, place=(0, "r16", "tight16"))
_case("pctl_one_more", 100, 60, data=("counts", COUNTS), lo=101, hi=501, place=(1, "plus1", "padded"))
_case("pctl_one_less", 100, 60, data=("counts", COUNTS), lo=99, hi=499)
_case("pctl_lo_eq_hi", 100, 60, data=("counts", COUNTS), lo=100, hi=100, prev=None)
_case("pctl_0_and_1000", 100, 60, data=("counts", COUNTS), lo=0, hi=1000, prev=None)
_case("pctl_1000_random", 100, 60, lo=1000, hi=1000)
# the mode: two values share the largest count -- the smaller one wins; the larger comes first in the picture
_case("mode_tie", 100, 60, data=("counts", [(250, 2500), (3, 2500), (100, 1000)]), prev=None)
# ---- prev holding 0xFFFFFFFF: a distance above 2^32
_case("prev_ones", 100, 60, n=2, prev="ones", cut=1000)
_case("prev_ones_roll", 17, 9, n=3, prev="ones", cut=1000, roll=1, place=(1, "plus1", "padded"))
# ---- selection: n across a wave of pictures; cuts and non-cuts interleaved so that every lane position selects at least once
for n in (1, 3, 64, 65, 130):
    _case("select_n%d" % n, 17, 3, n=n, prev="interleaved", cut=400, roll=n & 1, place=(0, "r16", "padded16") if n & 2 else (1, "tight", "tight"))
# ---- launches of thousands of work items, in which a wave takes several (hist_items_per_wave: items / 2048): 33 bands a picture, so
# the last wave of a picture has fewer items than the others
_case("many_items_2", 9, 260, n=130, prev="interleaved", cut=400, place=(0, "r16", "tight16"))
_case("many_items_4", 9, 260, n=260, data=("flat", 9), prev=None, place=(1, "tight", "tight"))
# ---- per-picture words (what h263mi_batch_hist_last hands the waves): an invalid picture, pictures in either frame set.  The plain
# entry point has no words: these run in the CPU checker, and on the GPU through the batch
_case("words_invalid_and_sets", 100, 60, n=4, prev="zero", cut=100, roll=1, place=(0, "r16", "padded16"), words=[VALID | SET1, 0, VALID, VALID | SET1])
_case("words_all_invalid", 33, 20, n=2, prev="ones", cut=0, roll=1, words=[0, 0])

# the cases the two mutants of the CPU checker must fail (test_sim_hist.py)
MUTANT_CASES = {
    "H263MI_MUTATE_HIST_CUT_CHUNK_FULL": ["size_1x1", "size_15x2", "size_17x9", "size_63x17", "size_1023x1", "size_1025x9", "size_2049x2",
                                          "place_0_r16_padded16_w100", "place_1_plus1_padded_w100", "place_4_r4_padded4_w100", "flat_255"],
    "H263MI_MUTATE_HIST_PERCENTILE_STRICT": ["pctl_exact", "pctl_lo_eq_hi", "pctl_0_and_1000", "ramp"],
}


class Built:
    pass


def _pitch(kind, w):
    return {"tight": w, "plus1": w + 1, "r16": (w + 15) // 16 * 16, "r4": (w + 15) // 16 * 16 + 4, "pitch256": (w + 255) // 256 * 256}[kind]


def _stride(kind, pitch, w, h):
    foot = h * pitch
    return {"tight": foot, "tight16": (foot + 15) // 16 * 16, "padded": foot + 37, "padded16": (foot + 15) // 16 * 16 + 48,
            "padded4": (foot + 3) // 4 * 4 + 20, "zero": 0, "rows2": 2 * pitch, "one": 1}[kind]


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


_decoded = []


def decoded_luma():
    """the luma planes of a decoded QCIF I picture and of the P picture behind it (recgen, the C oracle)"""
    if not _decoded:
        import recgen
        from oracle import oracle as orc
        mbs, coeffs = recgen.intra_picture(176, 144, seed=1)
        rc, first = orc.decode_picture(176, 144, mbs, coeffs, None)
        assert rc == 0
        mbs, coeffs = recgen.inter_picture(176, 144, seed=2, mv_range=40, p_4v=0.2, p_intra=0.1)
        rc, second = orc.decode_picture(176, 144, mbs, coeffs, first)
        assert rc == 0
        _decoded.extend([np.asarray(first[0], np.uint8).reshape(144, 176), np.asarray(second[0], np.uint8).reshape(144, 176)])
    return _decoded


def _fill(kind, p, w, h, rng):
    """picture p's pixels, or None: what the random buffer holds"""
    if kind == "random":
        return None
    if kind == "ramp":
        return ((np.arange(w * h) + 7 * p) % 256).astype(np.uint8).reshape(h, w)
    if kind == "decoded":
        return decoded_luma()[p % 2]
    if kind[0] == "flat":
        return np.full((h, w), kind[1], np.uint8)
    if kind[0] == "alt":
        _, what, a, b = kind
        y, x = np.mgrid[0:h, 0:w]
        sel = {"pixel": x + y + p, "16": x // 16 + p, "row": y + p}[what] & 1
        return np.where(sel, b, a).astype(np.uint8)
    if kind[0] == "counts":
        flat = np.concatenate([np.full(c, v, np.uint8) for v, c in kind[1]])
        assert flat.size == w * h
        if p:
            rng.shuffle(flat)                    # (picture 0 keeps the order of the list)
        return flat.reshape(h, w)
    raise KeyError(kind)


_built = {}


def build(name):
    if name in _built:
        return _built[name]
    cs = CASES[name]
    b = Built()
    b.name, b.w, b.h, b.n, b.roll, b.lo, b.hi, b.cut = name, cs["w"], cs["h"], cs["n"], cs["roll"], cs["lo"], cs["hi"], cs["cut"]
    b.pixels = b.w * b.h
    b.words = cs.get("words")
    b.valid = [bool(x & VALID) for x in b.words] if b.words else [True] * b.n
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    b.off, b.pitch, b.stride, nbytes, b.set1 = _place(cs["place"], b.w, b.h, b.n, 2 if b.words else 1)
    b.buf = rng.integers(0, 256, nbytes, dtype=np.uint8)
    b.at = [b.off + (b.set1 if b.words and b.words[p] & SET1 else 0) for p in range(b.n)]
    overlapping = b.n > 1 and b.stride < (b.h - 1) * b.pitch + b.w
    for p in range(b.n):
        px = _fill(cs["data"], p, b.w, b.h, rng)
        if px is not None and not (overlapping and p):       # (overlapping pictures share their bytes: the first one's stand)
            _rows(b.buf, b.at[p], b.pitch, b.stride, p, b.w, b.h)[:] = px
    b.planes = np.stack([_rows(b.buf, b.at[p], b.pitch, b.stride, p, b.w, b.h) for p in range(b.n)]).copy()
    b.hist = ref.histograms(b.planes)
    # prev: None, or (n, 256) uint32
    pk = cs["prev"]
    if pk is None:
        b.prev = None
    elif pk == "random":
        b.prev = rng.integers(0, 2 * b.pixels // 256 + 2, (b.n, 256)).astype(np.uint32)
    elif pk == "zero":
        b.prev = np.zeros((b.n, 256), np.uint32)
    elif pk == "ones":
        b.prev = np.full((b.n, 256), 0xFFFFFFFF, np.uint32)
    elif pk == "own":
        b.prev = b.hist.astype(np.uint32)
    elif pk == "interleaved":                                # cuts where p and its wave of 64 have the same parity: own / zero
        b.prev = b.hist.astype(np.uint32)
        for p in range(b.n):
            if p % 2 == (p // 64) % 2:
                b.prev[p] = 0
    elif pk[0] == "own_plus":
        b.prev = b.hist.astype(np.uint32)
        for p, add in enumerate(pk[1]):
            b.prev[p, 7] += add
    else:
        raise KeyError(pk)
    b.want_list = b.prev is not None
    b.buf.setflags(write=False)
    if b.prev is not None:
        b.prev.setflags(write=False)
    _built[name] = b
    return b


_expected = {}


def expected(b):
    """-> (the (n, 256) histograms, an invalid picture's zero; the statistics as tuples in hist_ref.stats' order; the selected indices;
    prev after the call, or None)"""
    if b.name not in _expected:
        hist = np.where(np.asarray(b.valid)[:, None], b.hist, 0).astype(np.uint32)
        st = [ref.stats(b.hist[p], b.prev[p] if b.prev is not None else None, b.lo, b.hi) if b.valid[p] else ref.ZERO_STATS for p in range(b.n)]
        sel = ref.select(st, b.cut, b.pixels, b.valid)
        after = None
        if b.prev is not None:
            after = b.prev.copy()
            if b.roll:
                for p in range(b.n):
                    if b.valid[p]:
                        after[p] = hist[p]
            after.setflags(write=False)
        _expected[b.name] = (hist, st, sel, after)
    return _expected[b.name]


def stats_tuples(raw):
    """a structured array of h263mi_hist_stats -> tuples in hist_ref.stats' order; the reserved bytes must be 0"""
    assert not raw["reserved"].any(), "reserved bytes written as non-zero"
    return [tuple(int(s[k]) for k in ("sum", "sum_sq", "distance", "min", "max", "p_lo", "p_hi", "mode")) for s in raw]


def compare(b, hist, prev, stats, lst, count):
    """None, or what differs from the reference.  hist (n, 256) uint32; prev (n, 256) after the call or None; stats: structured;
    lst: n words preset to SENTINEL, or None; count"""
    want_hist, want_stats, want_sel, want_prev = expected(b)
    if not (hist == want_hist).all():
        p, v = [int(x[0]) for x in np.nonzero(hist != want_hist)]
        return "hist[%d][%d]: %d, want %d" % (p, v, hist[p, v], want_hist[p, v])
    got = stats_tuples(stats)
    if got != want_stats:
        p = [i for i in range(b.n) if got[i] != want_stats[i]][0]
        return "stats[%d] %r, want %r" % (p, got[p], want_stats[p])
    if lst is not None:
        if count != len(want_sel) or lst[:count].tolist() != want_sel:
            return "list %r (%r), want %r" % (lst[:min(count, b.n)].tolist(), count, want_sel)
        if not (lst[count:] == SENTINEL).all():
            return "entries behind the count were written"
    if prev is not None and not (prev == want_prev).all():
        p, v = [int(x[0]) for x in np.nonzero(prev != want_prev)]
        return "prev[%d][%d]: %d, want %d" % (p, v, prev[p, v], want_prev[p, v])
    return None


def check_hazards():
    """On the reference alone: every hazard the table is there for occurs among its cases."""
    names = list(CASES)
    # widths on both sides of a chunk, of a segment and of two; heights of one row, of a short band, one above a band and one above
    # the two bands of a wave that takes two items; more than one picture count
    assert {CASES[n]["w"] for n in names} >= {1, 15, 16, 17, 63, 1023, 1024, 1025, 2049}
    assert {CASES[n]["h"] for n in names} >= {1, 2, 9, 2 * ROWS + 1}
    assert {CASES[n]["n"] for n in names} >= {1, 3, 64, 65, 130}
    # every load path, each with a whole last chunk and with one that the edge cuts; base and pitch 0, 1, 4 and 16 from a multiple of 16
    paths, offs, pitch_offs = set(), set(), set()
    for n in names:
        c = build(n)
        m = c.off | c.pitch | c.stride | c.set1
        paths.add((16 if m % 16 == 0 else 4 if m % 4 == 0 else 1, c.w % 16 != 0))
        offs.add(c.off % 16 if c.off < 16 else 16)
        pitch_offs.add((c.pitch - c.w) if c.pitch - c.w in (0, 1) else None)
    assert paths == {(a, cut) for a in (16, 4, 1) for cut in (False, True)}, paths
    assert offs >= {0, 1, 4, 16} and pitch_offs >= {0, 1}
    assert any(build(n).off == 4 and build(n).pitch % 16 == 4 for n in names)          # (the word path by its pitch too)
    # padding exists and is random: a count that took it in would differ
    assert any(build(n).pitch > build(n).w for n in names)
    # stride 0 and overlapping pictures
    s0 = build("stride_0")
    assert s0.stride == 0 and (s0.hist[0] == s0.hist[2]).all()
    for n in ("overlap_rows", "overlap_1"):
        o = build(n)
        assert 0 < o.stride < (o.h - 1) * o.pitch + o.w and not (o.hist[0] == o.hist[1]).all()
    # content: one bin holds P; two values; every value equally often; a decoded picture
    for v in (0, 255, 77):
        f = build("flat_%d" % v)
        assert f.hist[0, v] == f.pixels and expected(f)[1][0][3:] == (v, v, v, v, v)
    for n in ("alt_pixel", "alt_16", "alt_row"):
        a = build(n)
        assert (a.hist[0] > 0).sum() == 2 and (a.hist[1] > 0).sum() == 2
    assert build("alt_pixel").planes[0, 0, 0] != build("alt_pixel").planes[0, 0, 1]
    assert (build("alt_16").planes[0, 0, :16] == 0).all() and (build("alt_16").planes[0, 0, 16:32] == 255).all()
    assert (build("ramp").hist == 4).all() and (build("ramp_wide").hist == 10).all()
    d = build("decoded")
    assert (d.hist[0] > 0).sum() > 100 and not (d.hist[0] == d.hist[1]).all()
    big = build("flat_2048x1024")
    assert big.hist[0, 200] == 1 << 21 and big.h // ROWS * (big.w // SEG) == 256
    # the cut: a picture exactly on the bound is none, one count above is one
    c = build("cut_equal_and_above")
    st = expected(c)[1]
    assert [s[2] for s in st] == [3000, 3001, 2999, 0] and 3000 * 1000 == c.cut * 2 * c.pixels and expected(c)[2] == [1]
    assert expected(build("cut_0"))[2] == [1] and expected(build("cut_1000"))[2] == [1, 2]
    assert expected(build("cut_first_call"))[2] == [0, 1] and expected(build("cut_first_call_500"))[2] == []
    assert expected(build("cut_first_call"))[1][0][2] == 6000
    # percentiles: q * P == 1000 * C(v) exactly, and q one more and one less
    e = build("pctl_exact")
    for p in range(e.n):
        cum = np.cumsum(e.hist[p])
        assert 1000 * int(cum[10]) == e.lo * e.pixels and 1000 * int(cum[20]) == e.hi * e.pixels
    assert [s[5:7] for s in expected(e)[1]] == [(10, 20)] * 2
    assert [s[5:7] for s in expected(build("pctl_one_more"))[1]] == [(20, 200)] * 2
    assert [s[5:7] for s in expected(build("pctl_one_less"))[1]] == [(10, 20)] * 2
    assert [s[5:7] for s in expected(build("pctl_lo_eq_hi"))[1]] == [(10, 10)] * 2
    z = expected(build("pctl_0_and_1000"))[1][0]
    assert z[3:7] == (10, 200, 10, 200)                        # pctl(0) == min, pctl(1000) == max
    assert all(s[5] == s[6] == s[4] for s in expected(build("pctl_1000_random"))[1])
    assert [s[7] for s in expected(build("mode_tie"))[1]] == [3, 3] and build("mode_tie").planes[0, 0, 0] == 250
    # a distance above 2^32
    assert all(s[2] > 1 << 32 for s in expected(build("prev_ones"))[1])
    assert (expected(build("prev_ones_roll"))[3] == expected(build("prev_ones_roll"))[0]).all()
    # roll on and off, with and without prev and a list
    assert {(CASES[n]["roll"], CASES[n]["prev"] is None) for n in names} >= {(0, False), (1, False), (0, True)}
    # the selection crosses a wave of pictures, is not contiguous, and every lane position selects at least once
    s130 = expected(build("select_n130"))[2]
    assert {p % 64 for p in s130} == set(range(64)) and 0 < len(s130) < 130 and s130 == sorted(s130)
    assert any(p >= 64 for p in s130) and any(p >= 128 for p in s130)
    assert expected(build("select_n1"))[2] == [0] and expected(build("select_n3"))[2] == [0, 2]
    assert expected(build("select_n64"))[2] == list(range(0, 64, 2)) and expected(build("select_n65"))[2][-1] == 62
    # an invalid picture: all zero, never selected although its prev is far from zero, its prev kept
    wv = build("words_all_invalid")
    assert expected(wv)[2] == [] and not expected(wv)[0].any() and (expected(wv)[3] == 0xFFFFFFFF).all()
    wi = build("words_invalid_and_sets")
    assert expected(wi)[2] == [0, 2, 3] and expected(wi)[1][1] == ref.ZERO_STATS and wi.set1 > 0
    # launches in which a wave takes 2 and 4 items, 33 bands a picture
    for name, kk in (("many_items_2", 2), ("many_items_4", 4)):
        m = build(name)
        items = -(-m.h // ROWS) * -(-m.w // SEG)
        assert -(-m.h // ROWS) == 33 and (m.n * items) // 2048 == kk and items % kk
    # the mutants' cases: a cut chunk; a percentile reached exactly
    for n in MUTANT_CASES["H263MI_MUTATE_HIST_CUT_CHUNK_FULL"]:
        assert CASES[n]["w"] % 16
    for n in MUTANT_CASES["H263MI_MUTATE_HIST_PERCENTILE_STRICT"]:
        m = build(n)
        cum = np.cumsum(m.hist[0])
        assert any(1000 * int(cum[v]) == q * m.pixels for v in range(256) for q in (m.lo, m.hi))
