"""k_plane_resize (h263-rs_amd/csrc/plane_resize_kernel.inl) run lane by lane on the CPU under AddressSanitizer + UBSan
(tests/sim_yuv_resize/sim_yuv_resize.cpp), against the numpy restatement (yuv_resize_ref.py), byte for byte.  Every canvas byte
outside the planes' rectangles keeps its sentinel; a skipped picture writes nothing.  Both formats; tight pitches (odd: byte
stores) and padded ones that are multiples of 4 (word stores).  The division without a division instruction is checked at the
largest plane the library accepts: there a constant plane of 255 stays 255 and one of 0 stays 0."""
import os
import struct
import subprocess

import numpy as np
import pytest

import yuv_layout_ref as lay
import yuv_resize_ref as ref
from test_sim_rgba_resize import _largest_picture

HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = 0xC3
WAVE_COLUMNS = 256           # PLANE_OUT: output columns a wave covers in a row
# source -> output.  2100x3 -> 2x1: one output sample covers more source columns (1050) than one LDS hand-off holds (1024)
CASES = [((1, 1), (1, 1)), ((1, 1), (3, 2)), ((5, 4), (8, 9)), ((7, 9), (3, 2)), ((176, 144), (100, 37)), ((352, 288), (3, 2)),
         ((2100, 3), (2, 1)), ((300, 4), (WAVE_COLUMNS + 1, 3)), ((300, 4), (WAVE_COLUMNS - 1, 3)),
         ((96, 32), (2 * WAVE_COLUMNS + 2, 5)), ((64, 48), (32, 24))]
FORMATS = [lay.I420, lay.NV12]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    # built into a temporary directory: a read-only checkout passes too
    out = str(tmp_path_factory.mktemp("sim_yuv_resize") / "sim_yuv_resize")
    subprocess.check_call(["g++", "-O1", "-g", "-fno-strict-aliasing", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                           "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", out,
                           os.path.join(HERE, "sim_yuv_resize", "sim_yuv_resize.cpp")])
    return out


def _env():
    return dict(os.environ, ASAN_OPTIONS="detect_leaks=0")


def _run(driver, tmp, w, h, ow, oh, fmt, pitch_y, pitch_c, pictures, offsets, canvas):
    """offsets: 3 per picture (Y, Cb or CbCr, Cr), Y = 2^64 - 1: the picture is skipped"""
    inp, outp = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<8IQ", w, h, ow, oh, len(pictures), 1 if fmt == lay.NV12 else 0, pitch_y, pitch_c, canvas.size))
        f.write(np.asarray(offsets, np.uint64).tobytes())
        for p in pictures:
            for plane in p:
                f.write(plane.tobytes())
        f.write(canvas.tobytes())
    r = subprocess.run([driver, inp, outp], capture_output=True, text=True, env=_env(), timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.fromfile(outp, np.uint8)


def _pictures(rng, n, w, h):
    cw, ch = lay.chroma_size(w, h)
    return [tuple(rng.integers(0, 256, k, dtype=np.uint8) for k in (w * h, cw * ch, cw * ch)) for _ in range(n)]


def _pad4(v):
    return (v + 3) // 4 * 4 + 8


@pytest.mark.parametrize("fmt", FORMATS, ids=["i420", "nv12"])
@pytest.mark.parametrize("padded", [False, True], ids=["tight", "padded"])
@pytest.mark.parametrize("src,dst", CASES, ids=["%dx%d-%dx%d" % (s + d) for s, d in CASES])
def test_plane_resize_lane_by_lane(driver, tmp_path, src, dst, padded, fmt):
    (w, h), (ow, oh) = src, dst
    rng = np.random.default_rng(w * 7 + h * 13 + ow * 17 + oh + fmt)
    n = 3
    pics = _pictures(rng, n, w, h)
    ry, rc = lay.row_bytes(ow, fmt)
    if padded:
        py, pc = _pad4(ry), _pad4(rc)        # multiples of 4, default placement: every offset is one too (word stores)
    else:
        py, pc = ry, rc                       # tight: odd widths put planes on odd addresses (byte stores)
    oy, ocb, ocr = lay.default_offsets(n, ow, oh, fmt, py, pc)
    nbytes = n * lay.picture_bytes(ow, oh, fmt, py, pc)
    assert ref.extent(n, ow, oh, fmt, py, pc) == nbytes
    canvas = np.full(nbytes, SENTINEL, np.uint8)
    # the middle picture is skipped (a stream with nothing to render)
    offsets = []
    for s in range(n):
        offsets += [(1 << 64) - 1 if s == 1 else oy[s], ocb[s], 0 if ocr is None else ocr[s]]
    got = _run(driver, str(tmp_path), w, h, ow, oh, fmt, py, pc, pics, offsets, canvas)
    want = ref.place(np.full(nbytes, SENTINEL, np.uint8), [ref.resize_planes(p, w, h, ow, oh) for p in pics], ow, oh, fmt,
                     py, pc, oy, ocb, ocr, skip=(1,))
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "first differing byte %d of %d" % (bad[0], bad.size)


def test_wide_pitches_at_unaligned_offsets_take_the_byte_stores(driver, tmp_path):
    """pitches that are multiples of 4 with one plane at an odd offset: correct all the same"""
    (w, h), (ow, oh), fmt = (40, 30), (23, 11), lay.NV12
    rng = np.random.default_rng(5)
    pics = _pictures(rng, 1, w, h)
    py = pc = 64
    oy, ocb = [3], [3 + oh * py + 24]
    nbytes = ref.extent(1, ow, oh, fmt, py, pc, oy, ocb)
    assert nbytes is not None
    canvas = np.full(nbytes + 16, SENTINEL, np.uint8)
    got = _run(driver, str(tmp_path), w, h, ow, oh, fmt, py, pc, pics, [oy[0], ocb[0], 0], canvas)
    want = ref.place(np.full(canvas.size, SENTINEL, np.uint8), [ref.resize_planes(pics[0], w, h, ow, oh)], ow, oh, fmt, py, pc,
                     oy, ocb, None)
    assert (got == want).all()


@pytest.mark.parametrize("which", ["largest", "largest-1", "largest-chroma", "2^24", "2^24+1", "1", "2", "3", "1920x1080"])
def test_division_at_its_bound(driver, which):
    """resize_div at pw*ph = d for n = q*d - 1, q*d, q*d + d/2: with q = 255 and q = 0 the last is a constant plane"""
    big = _largest_picture()
    d = {"largest": big, "largest-1": big - 1, "largest-chroma": big // 4, "2^24": 1 << 24, "2^24+1": (1 << 24) + 1, "1": 1,
         "2": 2, "3": 3, "1920x1080": 1920 * 1080}[which]
    assert d < 1 << 30
    r = subprocess.run([driver, "--div", str(d)], capture_output=True, text=True, env=_env(), timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
