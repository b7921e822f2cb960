"""Framing of a resized output (h263mi_framing): h263mi_framing_resolve -- a pure host function, so all of this runs without a
device -- against the restatement in Python integers (framing_ref.py), which the hand-derived rectangles of
tests/golden/framing_known_answers.json pin; every refusal; and what must hold of every resolved framing."""
import ctypes as C
import json
import os

import pytest

import framing_ref as ref
import h263mi

GOLD = os.path.join(os.path.dirname(__file__), "golden", "framing_known_answers.json")
SOURCES = [(1, 1), (16, 16), (176, 144), (352, 288), (1920, 1080), (65535, 1)]
OUTPUTS = [(1, 1), (65, 5), (224, 224), (96, 64), (640, 640)]


def _cases():
    with open(GOLD) as f:
        return json.load(f)["cases"]


def _lib_resolve(w, h, ow, oh, f):
    """-> (rc, ((src), (dst))) of the library"""
    out = h263mi.FramingRects()
    rc = h263mi.lib().h263mi_framing_resolve(w, h, ow, oh, C.byref(f) if f is not None else None, C.byref(out))
    return rc, (out.src(), out.dst())


def _windows(w, h, ow, oh):
    """source and destination rectangles of a WINDOW for these sizes: whole, the last pixel, an inner rectangle"""
    for s, d in ((((0, 0, w, h)), (0, 0, ow, oh)), ((w - 1, h - 1, 1, 1), (ow - 1, oh - 1, 1, 1)),
                 ((w // 3, h // 3, (w + 1) // 2, (h + 1) // 2), (ow // 4, oh // 4, (ow + 1) // 2, (oh + 1) // 2))):
        yield s, d


def test_reference_matches_hand_derived_rectangles():
    names = set()
    for c in _cases():
        got = ref.resolve(c["w"], c["h"], c["ow"], c["oh"], ref.MODES[c["mode"]])
        assert got == (tuple(c["src"]), tuple(c["dst"])), (c["name"], got)
        names.add(c["name"])
    assert {"cif_letterbox_224", "1080p_letterbox_224", "cif_cover_224", "qcif_cover_96x64", "tie_rounds_half_up",
            "sliver_letterbox_clamps_to_one_row"} <= names


def test_library_matches_hand_derived_rectangles():
    for c in _cases():
        rc, got = _lib_resolve(c["w"], c["h"], c["ow"], c["oh"], h263mi.make_framing(ref.MODES[c["mode"]]))
        assert rc == h263mi.OK and got == (tuple(c["src"]), tuple(c["dst"])), (c["name"], rc, got)


@pytest.mark.parametrize("src", SOURCES, ids=["%dx%d" % s for s in SOURCES])
def test_resolve_sweep_against_reference_and_invariants(src):
    w, h = src
    for ow, oh in OUTPUTS:
        # a NULL framing is STRETCH
        rc, got = _lib_resolve(w, h, ow, oh, None)
        assert rc == h263mi.OK and got == ((0, 0, w, h), (0, 0, ow, oh))
        for mode in (ref.STRETCH, ref.LETTERBOX, ref.COVER):
            for keep in (0, 1):
                f = h263mi.make_framing(mode, pad=(114, 3, 255), keep_outside=keep)
                rc, got = _lib_resolve(w, h, ow, oh, f)
                want = ref.resolve(w, h, ow, oh, mode)
                assert rc == h263mi.OK and got == want, (w, h, ow, oh, mode, rc, got, want)
                (sx, sy, sw, sh), (dx, dy, dw, dh) = got
                # non-empty, inside their pictures
                assert sw >= 1 and sh >= 1 and dw >= 1 and dh >= 1
                assert sx + sw <= w and sy + sh <= h and dx + dw <= ow and dy + dh <= oh
                if mode == ref.STRETCH:
                    assert ref.whole(w, h, ow, oh, got)
                if mode == ref.LETTERBOX:
                    # the whole source; both edges of one axis touched, the other centred
                    assert (sx, sy, sw, sh) == (0, 0, w, h)
                    assert (dx == 0 and dw == ow) or (dy == 0 and dh == oh)
                    assert dx == (ow - dw) // 2 and dy == (oh - dh) // 2
                if mode == ref.COVER:
                    # the whole destination; one full axis of the source, the other centred
                    assert (dx, dy, dw, dh) == (0, 0, ow, oh)
                    assert (sx == 0 and sw == w) or (sy == 0 and sh == h)
                    assert sx == (w - sw) // 2 and sy == (h - sh) // 2
        for s, d in _windows(w, h, ow, oh):
            f = h263mi.make_framing(ref.WINDOW, src=s, dst=d)
            rc, got = _lib_resolve(w, h, ow, oh, f)
            assert rc == h263mi.OK and got == (s, d) == ref.resolve(w, h, ow, oh, ref.WINDOW, s, d)


def test_every_refusal():
    bad = h263mi.ERR_INVALID_ARGUMENT
    w, h, ow, oh = 176, 144, 96, 64
    L = h263mi.lib()
    ok = h263mi.make_framing(ref.LETTERBOX)
    out = h263mi.FramingRects()
    assert L.h263mi_framing_resolve(w, h, ow, oh, C.byref(ok), None) == bad               # nowhere to answer
    for sizes in ((0, h, ow, oh), (w, 0, ow, oh), (w, h, 0, oh), (w, h, ow, 0)):
        assert L.h263mi_framing_resolve(*sizes, C.byref(ok), C.byref(out)) == bad
        assert ref.resolve(*sizes, ref.LETTERBOX) is None
    f = h263mi.make_framing(4)
    assert _lib_resolve(w, h, ow, oh, f)[0] == bad and ref.resolve(w, h, ow, oh, 4) is None
    f = h263mi.make_framing(ref.COVER)
    f.keep_outside = 2
    assert _lib_resolve(w, h, ow, oh, f)[0] == bad and ref.resolve(w, h, ow, oh, ref.COVER, keep_outside=2) is None
    for k in range(3):
        f = h263mi.make_framing(ref.STRETCH)
        f.reserved[k] = 1
        assert _lib_resolve(w, h, ow, oh, f)[0] == bad
    assert ref.resolve(w, h, ow, oh, ref.STRETCH, reserved=(0, 0, 1)) is None
    # a rectangle field outside WINDOW, each of the eight
    for mode in (ref.STRETCH, ref.LETTERBOX, ref.COVER):
        for k in range(8):
            r = [0] * 8
            r[k] = 1
            f = h263mi.make_framing(mode, src=r[:4], dst=r[4:])
            assert _lib_resolve(w, h, ow, oh, f)[0] == bad, (mode, k)
            assert ref.resolve(w, h, ow, oh, mode, tuple(r[:4]), tuple(r[4:])) is None
    # WINDOW: an empty extent, a rectangle that leaves its picture
    good_s, good_d = (3, 5, 170, 131), (7, 3, 80, 33)
    assert _lib_resolve(w, h, ow, oh, h263mi.make_framing(ref.WINDOW, src=good_s, dst=good_d))[0] == h263mi.OK
    for s, d in (((3, 5, 0, 131), good_d), ((3, 5, 170, 0), good_d), (good_s, (7, 3, 0, 33)), (good_s, (7, 3, 80, 0)),
                 ((7, 5, 170, 131), good_d), ((3, 14, 170, 131), good_d), (good_s, (17, 3, 80, 33)), (good_s, (7, 32, 80, 33)),
                 ((176, 0, 1, 1), good_d), (good_s, (0, 64, 1, 1)), ((65535, 0, 65535, 1), good_d)):
        assert _lib_resolve(w, h, ow, oh, h263mi.make_framing(ref.WINDOW, src=s, dst=d))[0] == bad, (s, d)
        assert ref.resolve(w, h, ow, oh, ref.WINDOW, s, d) is None
    # a WINDOW with nothing given is empty
    assert _lib_resolve(w, h, ow, oh, h263mi.make_framing(ref.WINDOW))[0] == bad


def test_struct_layout():
    assert C.sizeof(h263mi.Framing) == 24 and C.sizeof(h263mi.FramingRects) == 16
    assert h263mi.Framing.src_x.offset == 8 and h263mi.Framing.dst_x.offset == 16 and h263mi.Framing.pad.offset == 2
