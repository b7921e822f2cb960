"""CPU side of the region tracks (h263mi_tracks_extent, h263mi_tracks_on, h263mi_batch_tracks): everything the host decides before
any device call -- the extent, every refusal include/h263mi.h lists, n_pictures == 0, and the device check behind them -- and the
reference itself: its two formulations of the greedy matching agree on every case and on 200 seeded random sequences.  The pointers
are made-up addresses: nothing here dereferences them, and a call that passes the argument checks names a device that no machine
has, so that it ends at the device check wherever the suite runs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import h263mi
import tracks_cases as tc
import tracks_ref as ref

BAD, OK, NO_DEVICE = h263mi.ERR_INVALID_ARGUMENT, h263mi.OK, h263mi.ERR_NO_DEVICE
NO_GPU = not os.path.exists("/dev/kfd")
NOWHERE = h263mi.BackendCfg(1 << 20, 0, None)                       # a device id beyond any machine's
ROIS, INFO_IN, STATE, CUT, CUT_COUNT, OUT, REFS, INFO, COUNT = (0x100000 * k for k in range(1, 10))
W, H, N, N_ROIS, MAX_OUT = 100, 60, 3, 50, 40
DEFAULT = object()
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "h263mi.h")


def call(rois=ROIS, n_rois=N_ROIS, info_in=INFO_IN, n=N, w=W, h=H, tracks=DEFAULT, state=STATE, state_bytes=None, cut=CUT,
         cut_count=CUT_COUNT, out=OUT, max_out=MAX_OUT, refs=REFS, info=INFO, count=COUNT):
    tracks = h263mi.make_tracks() if tracks is DEFAULT else tracks
    if state_bytes is None:
        state_bytes = n * (32 + 32 * (tracks.max_tracks if tracks is not None else 16))
    return h263mi.lib().h263mi_tracks_on(C.byref(NOWHERE), rois, n_rois, info_in, n, w, h, h263mi._opt(tracks), state, state_bytes, cut,
                                         cut_count, out, max_out, refs, info, count)


def test_the_structures_have_their_sizes():
    assert C.sizeof(h263mi.Tracks) == 16 and C.sizeof(h263mi.Track) == 32 and C.sizeof(h263mi.TrackHead) == 32
    assert C.sizeof(h263mi.TrackInfo) == 32 and C.sizeof(h263mi.TrackRef) == 16
    assert h263mi.TRACK_DTYPE.itemsize == 32 and h263mi.TRACK_HEAD_DTYPE.itemsize == 32 and h263mi.TRACK_INFO_DTYPE.itemsize == 32
    assert h263mi.TRACK_REF_DTYPE.itemsize == 16
    for name in ("h263mi_tracks_extent", "h263mi_tracks_on", "h263mi_batch_tracks"):
        assert name in h263mi.EXPORTS and hasattr(h263mi.lib(), name)
    assert h263mi.lib().h263mi_abi_version() == 7


def _header_struct(name):
    """the fields of `typedef struct name { ... }` in include/h263mi.h as [(C type, field name)]"""
    text = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            out += [(ctype, f.strip()) for f in names.split(",")]
    return out


def test_the_python_structures_and_the_reference_match_the_header():
    ctypes_of = {"uint8_t": C.c_uint8, "uint16_t": C.c_uint16, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
    for cname, cls in (("h263mi_tracks", h263mi.Tracks), ("h263mi_track", h263mi.Track), ("h263mi_track_head", h263mi.TrackHead),
                       ("h263mi_track_info", h263mi.TrackInfo), ("h263mi_track_ref", h263mi.TrackRef)):
        want = []
        for t, f in _header_struct(cname):
            m = re.fullmatch(r"(\w+)\[(\d+)\]", f)
            want.append((m.group(1), ctypes_of[t] * int(m.group(2))) if m else (f, ctypes_of[t]))
        assert [(f, C.sizeof(t)) for f, t in want] == [(f, C.sizeof(t)) for f, t in cls._fields_], cname
    for cls, dtype, mine in ((h263mi.Track, h263mi.TRACK_DTYPE, ref.TRACK), (h263mi.TrackHead, h263mi.TRACK_HEAD_DTYPE, ref.HEAD),
                             (h263mi.TrackInfo, h263mi.TRACK_INFO_DTYPE, ref.INFO), (h263mi.TrackRef, h263mi.TRACK_REF_DTYPE, ref.REF)):
        assert [(f, getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_] == \
            [(f, dtype.fields[f][1], dtype.fields[f][0].itemsize) for f in dtype.names]
        assert dtype == mine
    assert ref.ROI == h263mi.ROI_DTYPE and ref.INFO_IN == h263mi.REGION_INFO_DTYPE


def test_extent_values():
    t = h263mi.make_tracks
    assert h263mi.tracks_extent(3, 100, 60, t(16)) == 3 * (32 + 32 * 16)
    assert h263mi.tracks_extent(1, 1, 1, t(1)) == 64
    assert h263mi.tracks_extent(0, 8, 8, t()) == 0
    assert h263mi.tracks_extent(64, 1920, 1080, t(256)) == 64 * 8224
    assert h263mi.tracks_extent(65535, 4096, 4096, t(256)) == 65535 * 8224
    assert h263mi.lib().h263mi_tracks_extent(1, 8, 8, C.byref(t()), None) == OK          # the output pointer is optional


def test_extent_is_the_validator_of_the_description():
    ext = lambda n, w, h, t: h263mi.lib().h263mi_tracks_extent(n, w, h, h263mi._opt(t), None)
    t = h263mi.make_tracks
    assert ext(1, 8, 8, None) == BAD
    d = t()
    d.reserved = 1
    assert ext(1, 8, 8, d) == BAD
    assert ext(1, 8, 8, t(max_tracks=0)) == BAD and ext(1, 8, 8, t(max_tracks=257)) == BAD
    assert ext(1, 8, 8, t(max_tracks=1)) == OK and ext(1, 8, 8, t(max_tracks=256)) == OK
    assert ext(1, 8, 8, t(iou_permille=1001)) == BAD and ext(1, 8, 8, t(iou_permille=1000)) == OK and ext(1, 8, 8, t(iou_permille=0)) == OK
    assert ext(1, 8, 8, t(max_missed=65535)) == BAD and ext(1, 8, 8, t(max_missed=65534)) == OK and ext(1, 8, 8, t(max_missed=0)) == OK
    assert ext(1, 8, 8, t(min_hits=0)) == BAD and ext(1, 8, 8, t(min_hits=1)) == OK and ext(1, 8, 8, t(min_hits=65535)) == OK
    assert ext(1, 8, 8, t(emit_period=0xFFFFFFFF)) == OK
    assert ext(1, 0, 8, t()) == BAD and ext(1, 8, 0, t()) == BAD
    assert ext(1, 65536, 1, t()) == BAD and ext(1, 1, 65536, t()) == BAD and ext(1, 65535, 1, t()) == OK
    assert ext(1, 32768, 32768, t()) == BAD and ext(1, 32768, 32767, t()) == OK        # W*H >= 2^30
    assert ext(65536, 8, 8, t()) == BAD and ext(65535, 8, 8, t()) == OK


def test_refusals_of_the_call():
    t = h263mi.make_tracks
    assert call() == NO_DEVICE
    # anything the extent call refuses
    assert call(tracks=None) == BAD
    assert call(tracks=t(max_tracks=0)) == BAD and call(tracks=t(max_tracks=257)) == BAD and call(tracks=t(iou_permille=1001)) == BAD
    assert call(tracks=t(max_missed=65535)) == BAD and call(tracks=t(min_hits=0)) == BAD
    d = t()
    d.reserved = 7
    assert call(tracks=d) == BAD
    assert call(w=0) == BAD and call(h=0) == BAD and call(w=65536, h=1) == BAD and call(w=32768, h=32768) == BAD and call(n=65536) == BAD
    # a NULL that is needed
    assert call(info_in=None) == BAD and call(state=None) == BAD and call(out=None) == BAD and call(info=None) == BAD and call(count=None) == BAD
    assert call(rois=None) == BAD and call(rois=None, n_rois=0) == NO_DEVICE
    assert call(refs=None) == NO_DEVICE                                               # optional
    # n_rois, max_out
    assert call(n_rois=65536) == BAD and call(n_rois=65535) == NO_DEVICE and call(n_rois=0) == NO_DEVICE
    assert call(max_out=0) == BAD and call(max_out=65536) == BAD and call(max_out=1) == NO_DEVICE and call(max_out=65535) == NO_DEVICE
    # the state below its extent
    assert call(state_bytes=N * (32 + 32 * 16) - 1) == BAD and call(state_bytes=N * (32 + 32 * 16)) == NO_DEVICE
    assert call(tracks=t(256), state_bytes=N * 8224 - 1) == BAD and call(tracks=t(256), state_bytes=N * 8224) == NO_DEVICE
    # the cut list and its count: both or neither
    assert call(cut=None) == BAD and call(cut_count=None) == BAD and call(cut=None, cut_count=None) == NO_DEVICE
    # alignment: 4 bytes, the state 8
    for k in (1, 2, 3):
        for name, at in (("rois", ROIS), ("info_in", INFO_IN), ("cut", CUT), ("cut_count", CUT_COUNT), ("out", OUT), ("refs", REFS),
                         ("info", INFO), ("count", COUNT)):
            assert call(**{name: at + k}) == BAD, (name, k)
            assert call(**{name: at + 4}) == NO_DEVICE, name
    for k in (1, 2, 4, 7):
        assert call(state=STATE + k) == BAD
    assert call(state=STATE + 8) == NO_DEVICE


def test_an_output_may_not_intersect_an_input_or_another_output():
    sizes = {"rois": N_ROIS * 16, "info_in": N * 16, "cut": N * 4, "cut_count": 4, "state": N * (32 + 32 * 16), "out": MAX_OUT * 16,
             "refs": MAX_OUT * 16, "info": N * 32, "count": 8}
    outputs = ("state", "out", "refs", "info", "count")
    for out in outputs:
        for other in sizes:
            if other == out:
                continue
            base = 0x2000000
            # `out` begins inside `other`'s last bytes; then right behind it (the state at a multiple of 8)
            inside = (sizes[other] - 1) // 8 * 8 if out == "state" else sizes[other] - 4
            behind = -(-sizes[other] // 8) * 8 if out == "state" else sizes[other]
            assert call(**{other: base, out: base + inside}) == BAD, (out, other)
            assert call(**{other: base, out: base + behind}) == NO_DEVICE, (out, other)
            # `other` begins inside `out`'s last bytes
            assert call(**{out: base, other: base + sizes[out] - 4}) == BAD, (out, other)
            assert call(**{out: base, other: base + sizes[out]}) == NO_DEVICE, (out, other)
    # the inputs may share their bytes: they are only read
    assert call(rois=0x2000000, info_in=0x2000000, cut=0x2000000, cut_count=0x2000000) == NO_DEVICE
    # the state against the one word of the cut count that lies in its first and in its last bytes
    assert call(state=0x2000000, cut_count=0x2000000) == BAD and call(state=0x2000000, cut_count=0x2000000 + sizes["state"] - 4) == BAD


def test_an_earlier_refusal_wins_over_the_device_check_and_over_a_later_one():
    assert call(tracks=h263mi.make_tracks(max_tracks=300), info_in=None, n=70000, max_out=0) == BAD


def test_no_pictures_still_takes_a_device_for_the_table():
    assert call(n=0) == NO_DEVICE                                    # the table is filled, the counts become 0
    assert call(n=0, rois=None, n_rois=0, info_in=None, state=None, state_bytes=0, cut=None, cut_count=None, refs=None, info=None) == NO_DEVICE
    assert call(n=0, out=None) == BAD and call(n=0, count=None) == BAD and call(n=0, max_out=0) == BAD
    assert call(n=0, tracks=None) == BAD and call(n=0, w=0) == BAD and call(n=0, cut=None) == BAD


def test_the_batch_call_refuses_no_handle():
    t = h263mi.make_tracks()
    assert h263mi.lib().h263mi_batch_tracks(None, ROIS, N_ROIS, INFO_IN, C.byref(t), STATE, 1 << 20, None, None, OUT, MAX_OUT, None, INFO,
                                            COUNT) == BAD


@pytest.mark.skipif(not NO_GPU, reason="only meaningful where no GPU exists")
def test_a_valid_call_needs_a_device():
    t = h263mi.make_tracks()
    assert h263mi.lib().h263mi_tracks_on(None, ROIS, N_ROIS, INFO_IN, N, W, H, C.byref(t), STATE, 1 << 20, None, None, OUT, MAX_OUT, None,
                                         INFO, COUNT) == NO_DEVICE
    with pytest.raises(h263mi.H263Error) as e:
        h263mi.tracks(ROIS, N_ROIS, INFO_IN, N, W, H, t, STATE, 1 << 20, OUT, MAX_OUT, INFO, COUNT)
    assert e.value.code == NO_DEVICE


# ---------------------------------------------------------------------------------------------------------------------------
# the reference against itself
def _same(a, b):
    return all(tc.compare(x, *y) is None for x, y in zip(a, b)) and len(a) == len(b)


def test_every_hazard_occurs_among_the_cases():
    tc.check_hazards()


@pytest.mark.parametrize("name", list(tc.CASES))
def test_the_two_formulations_agree_on_every_case(name):
    k = tc.build(name)
    dbg = []
    assert _same(tc.expected(name), k.expected(ref.match_bruteforce, dbg))
    for per_call in dbg:
        for d in per_call:
            ref.check_matching(d["tracks"], d["dets"], k.prm.iou_permille, d["match"])
            assert tc.rounds_of_mutual_best(d["tracks"], d["dets"], k.prm.iou_permille)[1] == d["match"]


def test_the_two_formulations_agree_on_200_random_sequences():
    for seed in range(200):
        rng = np.random.default_rng(1000 + seed)
        k = tc.random_case(1000 + seed, n=int(rng.integers(1, 3)), max_tracks=int(rng.choice([1, 3, 7, 16])), calls=4,
                           w=160, h=120, objects=int(rng.integers(1, 14)), permille=int(rng.choice([0, 100, 300, 500])), dense=bool(seed & 1))
        dbg = []
        assert _same(k.expected(), k.expected(ref.match_bruteforce, dbg)), seed
        for per_call in dbg:
            for d in per_call:
                ref.check_matching(d["tracks"], d["dets"], k.prm.iou_permille, d["match"])
                assert tc.rounds_of_mutual_best(d["tracks"], d["dets"], k.prm.iou_permille)[1] == d["match"], seed
