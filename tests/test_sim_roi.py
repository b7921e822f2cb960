"""k_roi_tensor (h263-rs_amd/csrc/roi_kernel.inl) run lane by lane on the CPU under AddressSanitizer + UBSan
(tests/sim_roi/sim_roi.cpp: a stand-alone program), against the numpy reference (roi_ref: framing_ref.rgba of the WINDOW, then
tensor_out_ref.planes), as bit patterns.  The pictures are a buffer of exactly rgba_bytes, the output a canvas of sentinels in
which every byte that must not be written keeps its sentinel.  The tables are roi_cases.TABLES; that each hazard occurs among them
is asserted on the reference's side.  The device-made spans are compared against resize_spans, and resize_div is checked with a
reciprocal that is good to 1 ulp."""
import os
import struct
import subprocess

import numpy as np
import pytest

import roi_cases as rc
import roi_ref as ref
import tensor_out_ref as tref

HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = 0xC3
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    # built into a temporary directory: a read-only checkout passes too
    out = str(tmp_path_factory.mktemp("sim_roi") / "sim_roi")
    subprocess.check_call(["g++", "-O1", "-g", "-fno-strict-aliasing", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                           "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", out, os.path.join(HERE, "sim_roi", "sim_roi.cpp")])
    return out


_pictures, _crops = {}, {}


def table_pictures(name):
    if name not in _pictures:
        _pictures[name] = rc.pictures(name)
    return _pictures[name]


def table_crops(name):
    """crop() of every valid ROI of the table (None for the others): computed once per table, shared by the placements"""
    if name not in _crops:
        (w, h), n, _, (ow, oh), rois = rc.TABLES[name]
        _crops[name] = [ref.crop(table_pictures(name), r, ow, oh) if ref.valid(r, n, w, h) else None for r in rois]
    return _crops[name]


def run(driver, tmp, size, pics, out_size, rois, pl, canvas):
    """-> (the canvas after the launch, the status words)"""
    import h263mi
    (w, h), (ow, oh) = size, out_size
    inp, outp = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    table = rois if isinstance(rois, np.ndarray) else h263mi.roi_table(rois)
    with open(inp, "wb") as f:
        f.write(struct.pack("<8I", w, h, len(pics), ow, oh, pl["dtype"], 1 if pl["bgr"] else 0, len(table)))
        f.write(np.asarray(list(pl["scale"]) + list(pl["bias"]), np.float32).tobytes())
        f.write(struct.pack("<5Q", pl["stride_n"], pl["stride_c"], pl["stride_h"], pl["base"] * tref.ELT[pl["dtype"]], canvas.nbytes))
        f.write(table.tobytes())
        for p in pics:
            f.write(p.tobytes())
        f.write(canvas.tobytes())
    r = subprocess.run([driver, inp, outp], capture_output=True, text=True, env=ENV, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.fromfile(outp, np.uint8)
    return raw[:canvas.nbytes].view(canvas.dtype), raw[canvas.nbytes:].view(np.uint32)


def sentinel_canvas(pl):
    et = tref.BITS_DTYPE[pl["dtype"]]
    return np.full(pl["elements"], np.array([SENTINEL] * 4, np.uint8).view(et)[0], et)


def test_every_hazard_occurs_among_the_tables():
    met = set()
    for name in rc.TABLES:
        met |= rc.hazards(name)
    assert met == rc.ALL_HAZARDS, rc.ALL_HAZARDS ^ met
    assert {"one_column_last_segment", "one_row_last_band", "one_pixel_source", "invalid_x_plus_w_wraps_16_bits", "overlapping",
            "descending_pictures", "last_byte_of_the_buffer"} <= rc.hazards("qcif_65x5")
    assert "over_256_columns_odd_x" in rc.hazards("cif_wide_64x8")
    assert "identity" in rc.hazards("qcif_identity")
    assert {"byte_load_path", "last_byte_of_the_buffer"} <= rc.hazards("odd_width_33x7")
    assert "quotient_255" in rc.hazards("white_20x10")
    met = set()
    for which in rc.PLACEMENTS:
        met |= rc.placement_hazards(which)
    assert met == rc.ALL_PLACEMENT_HAZARDS
    # the white table does reach 255 in the reference
    assert all((c[:, :, :3] == 255).all() for c in table_crops("white_20x10"))


@pytest.mark.parametrize("which", list(rc.PLACEMENTS))
@pytest.mark.parametrize("name", list(rc.TABLES))
def test_tables_lane_by_lane(driver, tmp_path, name, which):
    size, n, _, out_size, rois = rc.TABLES[name]
    pl = rc.placement(name, which)
    canvas = sentinel_canvas(pl)
    got, status = run(driver, str(tmp_path), size, table_pictures(name), out_size, rois, pl, canvas)
    want, want_status = ref.expected(canvas, table_crops(name), rois, n, size[0], size[1], pl["dtype"], pl["scale"], pl["bias"], pl["bgr"],
                                     pl["base"], pl["stride_n"], pl["stride_c"], pl["stride_h"])
    assert (status == want_status).all(), (status, want_status)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "first differing element %d of %d: %#x, want %#x" % (bad[0], bad.size, got[bad[0]], want[bad[0]])
    assert (want != canvas).any() or not want_status.size or want_status.all()


def test_device_made_spans_equal_the_host_made_ones(driver):
    r = subprocess.run([driver, "--spans"], capture_output=True, text=True, env=ENV, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr


def test_resize_div_with_a_reciprocal_good_to_one_ulp(driver):
    # the largest divisors the entry point lets through: w*h < 2^30 with both sides at most 65535
    for d in ((1 << 30) - 1, 32768 * 32767, 65535 * 16384, 65535 * 16383, 1, 2, 3, 176 * 144):
        r = subprocess.run([driver, "--div", str(d)], capture_output=True, text=True, env=ENV, timeout=900)
        assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("which", ["f32_padded", "f16_odd_base_odd_stride"])
def test_garbage_tables_touch_nothing_outside_the_buffers(driver, tmp_path, which):
    """random 16-byte records -- wholly random, and random with `reserved` and `picture` cut down so that the rectangle decides:
    ASan sees any access outside the two buffers, the reference says which tensors are written"""
    name = "odd_width_33x7"
    size, n, _, out_size, _ = rc.TABLES[name]
    rng = np.random.default_rng(20250)
    table = rng.integers(0, 1 << 32, (192, 4), dtype=np.uint64).astype(np.uint32)
    table[32:, 3] = 0                                          # reserved
    table[32:, 0] %= 3                                         # picture 0..2 of 2
    table[64:, 1] &= 0x003f00ff                                # x < 256, y < 64
    table[64:, 2] &= 0x003f00ff                                # w < 256, h < 64
    table[96:, 1] &= 0x001f007f                                # x < 128, y < 32: most of these lie inside the 178 x 50 pictures
    table[96:, 2] &= 0x001f007f
    rois = [(int(r[0]), int(r[1] & 0xffff), int(r[1] >> 16), int(r[2] & 0xffff), int(r[2] >> 16), int(r[3])) for r in table]
    ok = [ref.valid(r, n, size[0], size[1]) for r in rois]
    assert 16 <= sum(ok) <= 90, sum(ok)
    pl = rc.placement(name, which, len(rois))
    canvas = sentinel_canvas(pl)
    pics = table_pictures(name)
    got, status = run(driver, str(tmp_path), size, pics, out_size, table, pl, canvas)
    crops = [ref.crop(pics, r, out_size[0], out_size[1]) if v else None for r, v in zip(rois, ok)]
    want, want_status = ref.expected(canvas, crops, rois, n, size[0], size[1], pl["dtype"], pl["scale"], pl["bias"], pl["bgr"], pl["base"],
                                     pl["stride_n"], pl["stride_c"], pl["stride_h"])
    assert (status == want_status).all()
    assert (got == want).all()
