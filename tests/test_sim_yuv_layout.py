"""The plane store of the YUV instantiations of the post kernels (post_kernel.inl: post_store_yuv, I420 and NV12, interior and
edge tiles) run lane by lane on the CPU under AddressSanitizer + UBSan (tests/sim_yuv/sim_yuv.cpp), against the oracle's
deblock() per plane put through the numpy restatement of the layout (tests/yuv_layout_ref.py).  Every canvas byte outside the
planes' rectangles keeps its sentinel."""
import os
import struct
import subprocess

import numpy as np
import pytest

import h263mi
import recgen
import simlib
import yuv_layout_ref as ref
from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(1, 1), (5, 4), (7, 9), (176, 144), (352, 288), (1920, 1080)]
SENTINEL = 0xC3


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    # built into a temporary directory: a read-only checkout passes too
    out = str(tmp_path_factory.mktemp("sim_yuv") / "sim_yuv")
    subprocess.check_call(["g++", "-O1", "-g", "-fno-strict-aliasing", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                           "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", out, os.path.join(HERE, "sim_yuv", "sim_yuv.cpp")])
    return out


def _run(driver, tmp, w, h, frames, strength, fmt, pitch_y, pitch_c, offs, canvas):
    """-> (canvas after the launch, tiles that took the interior path)"""
    oy, ocb, ocr = offs
    flat = []
    for s in range(len(frames)):
        flat += [oy[s], ocb[s], ocb[s] if ocr is None else ocr[s]]
    wide = int(pitch_y % 4 == 0 and pitch_c % 4 == 0 and all(o % 4 == 0 for o in flat))
    inp, outp = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<8IQ", w, h, len(frames), strength, 2 if fmt == ref.NV12 else 1, pitch_y, pitch_c, wide, canvas.size))
        f.write(np.asarray(flat, np.uint64).tobytes())
        for fr in frames:
            f.write(fr.tobytes())
        f.write(canvas.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([driver, inp, outp], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.fromfile(outp, np.uint8), int(r.stdout.strip())


def expected_planes(w, planes, strength):
    cw = (w + 1) // 2
    return planes if strength == 0 else tuple(orc.deblock(p, pw, strength) for p, pw in zip(planes, (w, cw, cw)))


def layouts(n, w, h, fmt):
    """name -> (pitch_y, pitch_c, (oy, ocb, ocr))"""
    ry, rc = ref.row_bytes(w, fmt)
    ch = (h + 1) // 2
    pad = lambda v: ((v + 255) // 256) * 256 + (256 if v % 256 == 0 else 0)
    out = {
        "tight": (ry, rc, ref.default_offsets(n, w, h, fmt)),
        "padded": (pad(ry), pad(rc), ref.default_offsets(n, w, h, fmt, pad(ry), pad(rc))),
    }
    # 2 x 2 mosaic with gaps on ONE grid: a tile is the luma, the Cb (or CbCr) plane below it, the Cr plane beside Cb;
    # 64 bytes between tile columns, a row between tile rows, 8 bytes in front and behind
    pitch = 2 * ry + 80
    assert fmt == ref.NV12 or 2 * rc + 4 <= ry + 64
    oy = [(p // 2) * (h + ch + 1) * pitch + (p % 2) * (ry + 64) + 8 for p in range(n)]
    ocb = [o + h * pitch for o in oy]
    ocr = None if fmt == ref.NV12 else [o + rc + 4 for o in ocb]
    out["mosaic"] = (pitch, pitch, (oy, ocb, ocr))
    return out


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("fmt", [ref.I420, ref.NV12])
def test_sim_yuv_layout(driver, tmp_path, w, h, fmt):
    L = simlib.layout(w, h)
    n = 4
    planes = [recgen.random_planes(w, h, 2000 + 7 * p + w) for p in range(n)]
    frames = [simlib.pack_frame(L, pl) for pl in planes]
    for strength in (0, 5, 12):
        want = [expected_planes(w, pl, strength) for pl in planes]
        for name, (py, pc, offs) in layouts(n, w, h, fmt).items():
            nbytes = ref.span_end(n, w, h, fmt, py, pc, *offs) + 16
            # (the library accepts the layout: h263mi_yuv_layout_extent needs no device)
            if name == "mosaic":
                assert h263mi.yuv_layout_extent(n, w, h, fmt, py, pc, *offs) == nbytes - 16
            else:
                assert h263mi.yuv_layout_extent(n, w, h, fmt, py, pc) == n * ref.picture_bytes(w, h, fmt, py, pc)
            canvas = np.full(nbytes, SENTINEL, np.uint8)
            got, interior = _run(driver, str(tmp_path), w, h, frames, strength, fmt, py, pc, offs, canvas)
            exp = ref.place(np.full(nbytes, SENTINEL, np.uint8), want, w, h, fmt, py, pc, *offs)
            bad = np.flatnonzero(got != exp)
            assert bad.size == 0, (name, strength, bad[:10], got[bad[:4]], exp[bad[:4]])
            assert (got[~ref.rect_mask(nbytes, n, w, h, fmt, py, pc, *offs)] == SENTINEL).all(), name
            # layouts of multiples of 4 take the interior path wherever the geometry allows it.  1080p: tile columns 1..14
            # of 1..15 (column 15 reaches x = 1924) and tile rows 1..32 of 0..33 (row 0 starts at y = -4, row 33 ends at 1084)
            if (w, h) == (1920, 1080):
                assert interior == n * 14 * 32, (name, interior)
            if (w, h) == (7, 9) or (name == "tight" and w % 4):
                assert interior == 0
