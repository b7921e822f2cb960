"""k_plane_filter (h263-rs_amd/csrc/plane_filter_kernel.inl) run lane by lane on the CPU under AddressSanitizer + UBSan
(tests/sim_plane_filter/sim_plane_filter.cpp: a stand-alone program), against the numpy reference (plane_filter_ref.planes:
Pillow's two-pass resampling per plane, restated), byte for byte.  Three pictures, the middle one skipped; I420 and NV12; three
placements (word stores; odd pitches and offsets; aligned pitches on a base that is 1 modulo 4); every canvas byte outside the
planes' rectangles keeps its sentinel.  The shapes are plane_filter_cases.CASES; that each hazard occurs among them is asserted
on the reference's side.  The same driver built with each of the two mutants of csrc/mutants.h must fail exactly where the
reference says it will, in luma and in chroma."""
import os
import struct
import subprocess

import numpy as np
import pytest

import filter_ref as flt
import plane_filter_cases as pc
import plane_filter_ref as ref
import yuv_layout_ref as lay
import yuv_resize_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = 0xC3
N = 3
SKIP = (1,)
MUTANTS = {"single": "-DH263MI_MUTATE_FILTER_SINGLE_ROUNDING", "mask": "-DH263MI_MUTATE_FILTER_NO_CLAMP"}
HAZARD_OF = {"single": "single_rounding_differs", "mask": "mask_differs"}
FORMATS = [lay.I420, lay.NV12]
PLACEMENTS = ["tight", "odd", "shifted"]
# the identity is the full-size layout on the host side: k_plane_filter never sees it
KERNEL_CASES = [name for name in pc.CASES if name != "identity"]


def _build(tmp_path_factory, name, *defines):
    # built into a temporary directory: a read-only checkout passes too
    out = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call(["g++", "-O1", "-g", "-fno-strict-aliasing", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                           "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", *defines, "-o", out,
                           os.path.join(HERE, "sim_plane_filter", "sim_plane_filter.cpp")])
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory, "sim_plane_filter")


@pytest.fixture(scope="module")
def mutant_drivers(tmp_path_factory):
    return {m: _build(tmp_path_factory, "sim_plane_filter_" + m, d) for m, d in MUTANTS.items()}


def _run(driver, tmp, name, kind, fmt, pitch_y, pitch_c, offs, base, canvas):
    (w, h), (ow, oh) = pc.CASES[name]
    oy, ocb, ocr = offs
    inp, outp = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    offsets = []
    for s in range(N):
        offsets += [(1 << 64) - 1 if s in SKIP else oy[s], ocb[s], 0 if ocr is None else ocr[s]]
    with open(inp, "wb") as f:
        f.write(struct.pack("<8I4IQ", w, h, ow, oh, N, 1 if fmt == lay.NV12 else 0, pitch_y, pitch_c, kind, base, 0, 0, canvas.size))
        f.write(np.asarray(offsets, np.uint64).tobytes())
        for s in range(N):
            for plane in pc.picture((w, h), s):
                f.write(plane.tobytes())
        f.write(canvas.tobytes())
    r = subprocess.run([driver, inp, outp], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"),
                       timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.fromfile(outp, np.uint8)


def _canvases(name, kind, fmt, placement, mutant=None):
    """(pitch_y, pitch_c, offsets, base, the sentinel canvas, the canvas as it must be afterwards)"""
    _, (ow, oh) = pc.CASES[name]
    py, pcc, offs, given, base, nbytes = ref.placements(ow, oh, fmt, N)[placement]
    assert yuv_resize_ref.extent(N, ow, oh, fmt, py, pcc, *(offs if given else (None, None, None))) is not None
    canvas = np.full(nbytes, SENTINEL, np.uint8)
    want = canvas.copy()
    ref.place(want[base:], [pc.want(name, kind, s, mutant) for s in range(N)], ow, oh, fmt, py, pcc, *offs, skip=SKIP)
    return py, pcc, offs, base, canvas, want


def test_every_hazard_occurs_among_the_cases():
    met, by_case = set(), {}
    for name in pc.CASES:
        for kind in pc.KINDS:
            hz = pc.geometry_hazards(name, kind)
            for s in range(N):
                if s not in SKIP:
                    hz = hz | pc.content_hazards(name, kind, s)
            by_case[(name, kind)] = hz
            met |= hz
    assert met == pc.ALL_HAZARDS, pc.ALL_HAZARDS - met
    # the device tests stop at CIF, whose chroma rows fit one chunk: everything else is met there too
    on_device = set().union(*(by_case[(name, kind)] for name in pc.GPU_CASES for kind in pc.KINDS))
    assert pc.ALL_HAZARDS - on_device == {"c_taps_over_one_chunk"}
    cubic = flt.BICUBIC
    assert {"y_taps_over_one_chunk", "y_coeff_rows_beyond_lds_cap", "c_coeff_rows_beyond_lds_cap", "last_segment_one_column",
            "last_band_one_row"} <= by_case[("cif_1x1", cubic)]
    assert {"last_segment_one_column", "last_band_one_row", "chroma_last_band_short"} <= by_case[("qcif_257x5", cubic)]
    assert pc.CASES["qcif_257x5"][1][0] % pc.COLS_PER_SEGMENT == 1 and (pc.CASES["qcif_257x5"][1][1] + 1) // 2 == 3
    assert "horizontal_skipped" in by_case[("qcif_176x97", cubic)] and "vertical_skipped" in by_case[("qcif_129x144", cubic)]
    assert {"chroma_horizontal_skipped_only", "chroma_wholly_skipped"} <= by_case[("qcif_175x144", cubic)]
    assert {"chroma_vertical_skipped_only", "chroma_wholly_skipped"} <= by_case[("qcif_176x143", cubic)]
    assert {"odd_source", "unaligned_chroma_rows"} <= by_case[("odd_40x30", cubic)] and "odd_source" in by_case[("odd_224", cubic)]
    assert "luma_beyond_lds_cap_chroma_within" in by_case[("qcif_25x144", flt.BILINEAR)]
    assert "c_taps_over_one_chunk" in by_case[("wide_5x3", cubic)]
    assert by_case[("identity", cubic)] == {"full_size"}
    # bilinear weights are never negative: nothing leaves 0..255; the cubic clamps on both sides in both passes of luma and chroma
    clamps = {p + "_" + a + "_clamp_" + v for p in pc.PLANES for a in "hv" for v in ("0", "255")}
    for (name, kind), hz in by_case.items():
        if kind == flt.BILINEAR:
            assert not hz & (clamps | {"y_mask_differs", "c_mask_differs"}), name
    assert clamps <= by_case[("qcif_224", cubic)]
    # 1 x 1 reaches no clamp
    assert not by_case[("cif_1x1", cubic)] & clamps


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("fmt", FORMATS, ids=["i420", "nv12"])
@pytest.mark.parametrize("kind", pc.KINDS, ids=pc.KIND_IDS)
@pytest.mark.parametrize("name", KERNEL_CASES)
def test_plane_filter_lane_by_lane(driver, tmp_path, name, kind, fmt, placement):
    py, pcc, offs, base, canvas, want = _canvases(name, kind, fmt, placement)
    got = _run(driver, str(tmp_path), name, kind, fmt, py, pcc, offs, base, canvas)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "first differing byte %d of %d: %#x, want %#x" % (bad[0], bad.size, got[bad[0]], want[bad[0]])


def _plane_differs(got, want, name, fmt, py, pcc, offs, base):
    """(a luma byte differs, a chroma byte differs)"""
    _, (ow, oh) = pc.CASES[name]
    luma = np.zeros(got.size, bool)
    ry, _ = lay.row_bytes(ow, fmt)
    for s in range(N):
        for r in range(oh):
            at = base + offs[0][s] + r * py
            luma[at:at + ry] = True
    bad = got != want
    return bool((bad & luma).any()), bool((bad & ~luma).any())


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutant_fails_where_the_reference_says(mutant_drivers, tmp_path, mutant):
    """every case and kind through the mutant build, NV12 with word stores: it computes what the reference computes with the same
    mutation, so it differs from the contract exactly at the cases and in the planes whose pictures meet the mutant's hazard --
    and some do, in luma and in chroma"""
    failed = {"y": [], "c": []}
    fmt, placement = lay.NV12, "tight"
    for name in KERNEL_CASES:
        for kind in pc.KINDS:
            py, pcc, offs, base, canvas, want = _canvases(name, kind, fmt, placement)
            got = _run(mutant_drivers[mutant], str(tmp_path), name, kind, fmt, py, pcc, offs, base, canvas)
            hz = set().union(*(pc.content_hazards(name, kind, s) for s in range(N) if s not in SKIP))
            expect = ("y_" + HAZARD_OF[mutant] in hz, "c_" + HAZARD_OF[mutant] in hz)
            assert _plane_differs(got, want, name, fmt, py, pcc, offs, base) == expect, (name, kind, expect)
            assert (got == _canvases(name, kind, fmt, placement, mutant)[5]).all(), (name, kind)
            for p, hit in zip("yc", expect):
                if hit:
                    failed[p].append((name, kind))
    assert len(failed["y"]) >= 4 and len(failed["c"]) >= 4, failed
    if mutant == "mask":
        assert all(kind == flt.BICUBIC for p in "yc" for _, kind in failed[p])
    # a skipped pass leaves one rounding: nothing for the single-rounding mutant to change
    if mutant == "single":
        assert not {n for p in "yc" for n, _ in failed[p]} & {"qcif_176x97", "qcif_129x144", "qcif_25x144"}
        assert "qcif_175x144" not in {n for n, _ in failed["c"]} and "qcif_176x143" not in {n for n, _ in failed["c"]}
