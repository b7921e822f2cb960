"""k_rgba_filter and k_tensor_filter (h263-rs_amd/csrc/filter_kernel.inl) run lane by lane on the CPU under AddressSanitizer +
UBSan (tests/sim_filter/sim_filter.cpp: a stand-alone program), against the numpy reference (filter_ref.rgba: Pillow's two-pass
resampling of the source window pasted into a canvas of the pad colour; tensor_out_ref.planes), as bit patterns.  Three pictures
at padded strides, the middle one skipped; with pad and with keep_outside; every canvas byte that must not be written keeps its
sentinel.  The shapes are filter_cases.CASES; that each hazard occurs among them is asserted on the reference's side.  The same
driver built with each of the two mutants of csrc/mutants.h must fail exactly where the reference says it will."""
import os
import struct
import subprocess

import numpy as np
import pytest

import filter_cases as fc
import filter_ref as ref
import framing_ref as fref
import tensor_out_ref as tref

HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = 0xC3
PAD = (114, 7, 250)
RGBA = 3
MUTANTS = {"single": "-DH263MI_MUTATE_FILTER_SINGLE_ROUNDING", "mask": "-DH263MI_MUTATE_FILTER_NO_CLAMP"}
HAZARD_OF = {"single": "single_rounding_differs", "mask": "mask_differs"}


def _build(tmp_path_factory, name, *defines):
    # built into a temporary directory: a read-only checkout passes too
    out = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call(["g++", "-O1", "-g", "-fno-strict-aliasing", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                           "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", *defines, "-o", out, os.path.join(HERE, "sim_filter", "sim_filter.cpp")])
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory, "sim_filter")


@pytest.fixture(scope="module")
def mutant_drivers(tmp_path_factory):
    return {m: _build(tmp_path_factory, "sim_filter_" + m, d) for m, d in MUTANTS.items()}


@pytest.fixture(scope="module")
def pictures():
    """three full-size pictures per source size, made once"""
    return {size: [fc.picture(size, k) for k in range(3)] for size in (fc.QCIF, fc.CIF)}


_want = {}


def want_rgba(name, kind, pictures, mutant=None):
    """the W' x H' RGBA of the case's pictures 0 and 2 with the pad colour around: computed once per case and kind"""
    key = (name, kind, mutant)
    if key not in _want:
        size, (ow, oh), _, _, _ = fc.CASES[name]
        _want[key] = {s: ref.rgba(pictures[size][s], ow, oh, fc.rects(name), kind, PAD, mutant=mutant) for s in (0, 2)}
    return _want[key]


def _run(driver, tmp, name, kind, pics, dtype, bgr, keep, pitch, scale, bias, stride_c, stride_h, offsets, canvas):
    (w, h), (ow, oh), _, _, _ = fc.CASES[name]
    s, d = fc.rects(name)
    inp, outp = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<8I", w, h, ow, oh, len(pics), dtype, 1 if bgr else 0, 1 if keep else 0))
        f.write(struct.pack("<8I", *(s + d)))
        f.write(struct.pack("<4I", PAD[0] | PAD[1] << 8 | PAD[2] << 16, pitch, kind, 0))
        f.write(np.asarray(list(scale) + list(bias), np.float32).tobytes())
        f.write(struct.pack("<3Q", stride_c, stride_h, canvas.nbytes))
        f.write(np.asarray(offsets, np.uint64).tobytes())
        for p in pics:
            f.write(p.tobytes())
        f.write(canvas.tobytes())
    r = subprocess.run([driver, inp, outp], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"),
                       timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.fromfile(outp, canvas.dtype)


def test_every_hazard_occurs_among_the_cases(pictures):
    met, by_case = set(), {}
    for name in fc.CASES:
        size = fc.CASES[name][0]
        for kind in fc.KINDS:
            hz = fc.geometry_hazards(name, kind)
            for s in (0, 2):
                hz |= fc.content_hazards(name, kind, pictures[size][s])
            by_case[(name, kind)] = hz
            met |= hz
    assert met == fc.ALL_HAZARDS, fc.ALL_HAZARDS - met
    assert {"taps_over_256_columns", "last_band_one_row", "last_segment_one_column"} <= by_case[("cif_1x1", ref.BICUBIC)]
    assert "last_segment_one_column" in by_case[("qcif_65x5", ref.BILINEAR)] and fc.CASES["qcif_65x5"][1][1] % fc.ROWS_PER_BAND == 1
    assert "horizontal_skipped" in by_case[("qcif_176x97", ref.BICUBIC)] and "vertical_skipped" in by_case[("qcif_129x144", ref.BICUBIC)]
    assert {"odd_sx", "taps_over_256_columns", "framed"} <= by_case[("cif_window_300", ref.BILINEAR)]
    assert "shared_tap_window" in by_case[("qcif_224", ref.BILINEAR)]
    # bilinear weights are never negative: nothing leaves 0..255; the cubic clamps on both sides in both passes
    for (name, kind), hz in by_case.items():
        if kind == ref.BILINEAR:
            assert not hz & {"h_clamp_0", "h_clamp_255", "v_clamp_0", "v_clamp_255", "mask_differs"}, name
    assert {"h_clamp_0", "h_clamp_255", "v_clamp_0", "v_clamp_255"} <= by_case[("qcif_224", ref.BICUBIC)]


def _rgba_canvas(name, kind, keep, pictures, mutant=None):
    """(pitch, offsets, the sentinel canvas, the canvas as it must be afterwards)"""
    _, (ow, oh), _, _, _ = fc.CASES[name]
    pitch = 4 * ow + 8
    stride = oh * pitch + 12
    canvas = np.full(4 + 3 * stride, SENTINEL, np.uint8)
    offsets = [4 + s * stride for s in range(3)]
    offsets[1] = (1 << 64) - 1                                       # the middle picture: nothing to render
    want = canvas.copy()
    mask = fref.inside(fc.rects(name), oh, ow)
    for s in (0, 2):
        pic = want_rgba(name, kind, pictures, mutant)[s]
        for y in range(oh):
            at = 4 + s * stride + y * pitch
            row = want[at:at + 4 * ow].reshape(ow, 4)
            sel = mask[y] if keep else np.ones(ow, bool)
            row[sel] = pic[y][sel]
    return pitch, offsets, canvas, want


@pytest.mark.parametrize("keep", [False, True], ids=["pad", "keep"])
@pytest.mark.parametrize("kind", fc.KINDS, ids=fc.KIND_IDS)
@pytest.mark.parametrize("name", list(fc.CASES))
def test_rgba_lane_by_lane(driver, pictures, tmp_path, name, kind, keep):
    pitch, offsets, canvas, want = _rgba_canvas(name, kind, keep, pictures)
    got = _run(driver, str(tmp_path), name, kind, pictures[fc.CASES[name][0]], RGBA, False, keep, pitch, (1, 1, 1), (0, 0, 0), 0, 0,
               offsets, canvas)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "first differing byte %d of %d: %#x, want %#x" % (bad[0], bad.size, got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("keep", [False, True], ids=["pad", "keep"])
@pytest.mark.parametrize("dtype", [tref.F32, tref.F16, tref.BF16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("kind", fc.KINDS, ids=fc.KIND_IDS)
@pytest.mark.parametrize("name", list(fc.CASES))
def test_tensor_lane_by_lane(driver, pictures, tmp_path, name, kind, dtype, keep):
    size, (ow, oh), _, _, _ = fc.CASES[name]
    bgr = dtype == tref.F16
    scale, bias = tref.EDGES if dtype == tref.F16 else tref.IMAGENET
    # padded strides (an odd stride_h: the rows of a 16-bit tensor alternate between aligned and not); the base one element into
    # the canvas: an odd element index
    stride_h = ow + 3 if (ow + 3) % 2 else ow + 4
    stride_c = oh * stride_h + 5
    stride_n = 3 * stride_c + 7
    et = tref.BITS_DTYPE[dtype]
    sent = np.array([SENTINEL] * 4, np.uint8).view(et)[0]
    mask = fref.inside(fc.rects(name), oh, ow)
    base = 1
    n_elem = base + 2 * stride_n + 2 * stride_c + (oh - 1) * stride_h + ow + 9
    canvas = np.full(n_elem, sent, et)
    offsets = [(base + s * stride_n) * tref.ELT[dtype] for s in range(3)]
    offsets[1] = (1 << 64) - 1
    got = _run(driver, str(tmp_path), name, kind, pictures[size], dtype, bgr, keep, 0, scale, bias, stride_c, stride_h, offsets, canvas)
    want = canvas.copy()
    for s in (0, 2):
        pl = tref.planes(want_rgba(name, kind, pictures)[s], dtype, scale, bias, bgr)
        for p in range(3):
            for y in range(oh):
                at = base + s * stride_n + p * stride_c + y * stride_h
                sel = mask[y] if keep else np.ones(ow, bool)
                want[at:at + ow][sel] = pl[p, y][sel]
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "first differing element %d of %d: %#x, want %#x" % (bad[0], bad.size, got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutant_fails_where_the_reference_says(mutant_drivers, pictures, tmp_path, mutant):
    """every case and kind as RGBA through the mutant build: it computes what the reference computes with the same mutation, so
    it differs from the contract exactly at the cases whose pictures meet the mutant's hazard -- and some do"""
    failed = []
    for name in fc.CASES:
        size = fc.CASES[name][0]
        for kind in fc.KINDS:
            pitch, offsets, canvas, want = _rgba_canvas(name, kind, False, pictures)
            got = _run(mutant_drivers[mutant], str(tmp_path), name, kind, pictures[size], RGBA, False, False, pitch, (1, 1, 1), (0, 0, 0),
                       0, 0, offsets, canvas)
            hazard = any(HAZARD_OF[mutant] in fc.content_hazards(name, kind, pictures[size][s]) for s in (0, 2))
            assert bool((got != want).any()) == hazard, (name, kind, hazard)
            assert (got == _rgba_canvas(name, kind, False, pictures, mutant)[3]).all(), (name, kind)
            if hazard:
                failed.append((name, kind))
    assert len(failed) >= 6, failed
    if mutant == "mask":
        assert all(kind == ref.BICUBIC for _, kind in failed)
    # a skipped pass leaves one rounding: nothing for the single-rounding mutant to change
    if mutant == "single":
        assert not {n for n, _ in failed} & {"qcif_176x97", "qcif_129x144", "qcif_one_pixel"}
