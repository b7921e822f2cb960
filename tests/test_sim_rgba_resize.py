"""k_rgba_resize (h263-rs_amd/csrc/resize_kernel.inl) run lane by lane on the CPU under AddressSanitizer + UBSan
(tests/sim_resize/sim_resize.cpp), against the numpy restatement (rgba_resize_ref.py).  Every canvas byte outside the
pictures' rectangles keeps its sentinel; a skipped picture writes nothing.  The division without a division instruction is
checked at the largest picture the library accepts."""
import os
import struct
import subprocess

import numpy as np
import pytest

import rgba_resize_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = 0xC3
CASES = [((1, 1), (1, 1)), ((1, 1), (7, 5)), ((7, 9), (3, 4)), ((176, 144), (480, 270)), ((1920, 1080), (640, 360)),
         ((1920, 1080), (1, 1)), ((352, 288), (352, 1))]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    # built into a temporary directory: a read-only checkout passes too
    out = str(tmp_path_factory.mktemp("sim_resize") / "sim_resize")
    subprocess.check_call(["g++", "-O1", "-g", "-fno-strict-aliasing", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                           "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", out, os.path.join(HERE, "sim_resize", "sim_resize.cpp")])
    return out


def _env():
    return dict(os.environ, ASAN_OPTIONS="detect_leaks=0")


def _run(driver, tmp, w, h, ow, oh, pictures, pitch, offsets, canvas):
    inp, outp = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<6IQ", w, h, ow, oh, len(pictures), pitch, canvas.size))
        f.write(np.asarray(offsets, np.uint64).tobytes())
        for p in pictures:
            f.write(p.tobytes())
        f.write(canvas.tobytes())
    r = subprocess.run([driver, inp, outp], capture_output=True, text=True, env=_env(), timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.fromfile(outp, np.uint8)


@pytest.mark.parametrize("src,dst", CASES, ids=["%dx%d-%dx%d" % (s + d) for s, d in CASES])
def test_resize_lane_by_lane(driver, tmp_path, src, dst):
    (w, h), (ow, oh) = src, dst
    rng = np.random.default_rng(w * 7 + h * 13 + ow * 17 + oh)
    pics = [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for _ in range(3)]
    for p in pics:
        p[:, :, 3] = 255
    # three pictures side by side at a pitch wider than the three rows; the middle one is skipped (nothing to render)
    row = 4 * ow
    pitch = 3 * row + 12
    offsets = [0, row, 2 * row + 8]
    nbytes = (oh - 1) * pitch + offsets[2] + row + 64
    canvas = np.full(nbytes, SENTINEL, np.uint8)
    sent = list(offsets)
    sent[1] = (1 << 64) - 1
    got = _run(driver, str(tmp_path), w, h, ow, oh, pics, pitch, sent, canvas)
    want = np.full(nbytes, SENTINEL, np.uint8)
    for s in (0, 2):
        out = ref.resize(pics[s], w, h, ow, oh)
        for r in range(oh):
            want[offsets[s] + r * pitch: offsets[s] + r * pitch + row] = out[r].ravel()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "first differing byte %d of %d" % (bad[0], bad.size)


def _largest_picture():
    """the largest w*h that layout_fits accepts (dev_common.h): w, h <= 65535, one frame <= 2^30 bytes"""
    best = 0
    for w in range(1, 65536):
        mbw = (w + 15) // 16
        pitch_c = ((mbw * 8 + 63) // 64) * 64
        # bytes = 48 * pitch_c * mbh + 512 <= 2^30
        mbh = min((((1 << 30) - 512) // (48 * pitch_c)), 65535 // 16 + 1)
        h = min(65535, mbh * 16)
        best = max(best, w * h)
    return best


def test_largest_picture_is_about_700_mpixels():
    d = _largest_picture()
    assert 700e6 < d < 2 ** 30


@pytest.mark.parametrize("which", ["largest", "largest-1", "2^24", "2^24+1", "1", "2", "3", "1920x1080"])
def test_division_at_its_bound(driver, which):
    big = _largest_picture()
    d = {"largest": big, "largest-1": big - 1, "2^24": 1 << 24, "2^24+1": (1 << 24) + 1, "1": 1, "2": 2, "3": 3,
         "1920x1080": 1920 * 1080}[which]
    r = subprocess.run([driver, "--div", str(d)], capture_output=True, text=True, env=_env(), timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
