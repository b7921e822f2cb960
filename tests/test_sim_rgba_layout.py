"""The scaled / pitched RGBA store of the post kernels (post_kernel.inl: post_phase_store with SCALE >= 0) run lane by
lane on the CPU under AddressSanitizer + UBSan (tests/sim_layout/sim_layout.cpp), against the numpy restatement applied to
the oracle's full-size RGBA.  Every canvas byte outside the pictures' rectangles keeps its sentinel."""
import os
import struct
import subprocess

import numpy as np
import pytest

import recgen
import rgba_layout_ref as ref
import simlib
from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(1, 1), (5, 4), (7, 9), (176, 144), (352, 288), (1920, 1080)]
SENTINEL = 0xC3


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    # built into a temporary directory: a read-only checkout passes too
    out = str(tmp_path_factory.mktemp("sim_layout") / "sim_layout")
    subprocess.check_call(["g++", "-O1", "-g", "-fno-strict-aliasing", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                           "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", out, os.path.join(HERE, "sim_layout", "sim_layout.cpp")])
    return out


def _run(driver, tmp, w, h, frames, strength, scale, pitch, offsets, canvas):
    inp, outp = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<6IQ", w, h, len(frames), strength, scale, pitch, canvas.size))
        f.write(np.asarray(offsets, np.uint64).tobytes())
        for fr in frames:
            f.write(fr.tobytes())
        f.write(canvas.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([driver, inp, outp], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.fromfile(outp, np.uint8)


def _expected_rgba(w, h, planes, strength):
    cw = (w + 1) // 2
    filt = planes if strength == 0 else tuple(orc.deblock(p, pw, strength) for p, pw in zip(planes, (w, cw, cw)))
    return orc.yuv420_to_rgba(*filt, w)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("scale", [0, 1, 2])
def test_sim_layout(driver, tmp_path, w, h, scale):
    L = simlib.layout(w, h)
    n = 4
    planes = [recgen.random_planes(w, h, 1000 + 7 * p + w) for p in range(n)]
    frames = [simlib.pack_frame(L, pl) for pl in planes]
    ow, oh = ref.out_size(w, h, scale)
    for strength in (0, 5, 12):
        want = [ref.box_average(_expected_rgba(w, h, pl, strength), w, h, scale) for pl in planes]
        tight = 4 * ow
        padded = ((tight + 255) // 256) * 256 + (256 if tight % 256 == 0 else 0)
        mosaic_pitch = 2 * tight + 64                                     # 2 x 2 tiles, 16 pixels of gap between columns
        layouts = {
            "tight": (tight, ref.default_offsets(n, w, h, scale)),
            "padded": (padded, ref.default_offsets(n, w, h, scale, padded)),
            "mosaic": (mosaic_pitch, [(p // 2) * (oh + 1) * mosaic_pitch + (p % 2) * (tight + 64) + 8 for p in range(n)]),
        }
        for name, (pitch, offs) in layouts.items():
            nbytes = max(o + (oh - 1) * pitch + tight for o in offs) + 16
            canvas = np.full(nbytes, SENTINEL, np.uint8)
            got = _run(driver, str(tmp_path), w, h, frames, strength, scale, pitch, offs, canvas)
            exp = ref.place(np.full(nbytes, SENTINEL, np.uint8), want, pitch, offs)
            bad = np.flatnonzero(got != exp)
            assert bad.size == 0, (name, strength, bad[:10], got[bad[:4]], exp[bad[:4]])
            assert (got[~ref.rect_mask(nbytes, w, h, scale, pitch, offs)] == SENTINEL).all(), name
