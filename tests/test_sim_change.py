"""k_change and k_change_select (change_wave, change_select: h263-rs_amd/csrc/change_kernel.inl) run lane by lane on the CPU under AddressSanitizer + UBSan
(tests/sim_change/sim_change.cpp: a stand-alone program, run as a child process), against the numpy reference (change_ref), exactly.
cur and prev are heap buffers of exactly the sets' bytes, the grids, the summaries and the list buffers of exactly their extents:
ASan sees any access outside, and inside them every byte that must not change keeps its value.  The cases are
change_cases.CASES; that each hazard occurs among them is asserted on the reference's side.  The two mutants of mutants.h must
fail the cases named for them."""
import os
import struct
import subprocess

import numpy as np
import pytest

import change_cases as cc

HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = 0xC3C3C3C3
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
SUMMARY = np.dtype([("sad", np.uint64), ("changed_cells", np.uint32), ("max_cell_sad", np.uint32)])


def build_driver(out, *defines):
    subprocess.check_call(["g++", "-O1", "-g", "-fno-strict-aliasing", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *["-D" + d for d in defines], "-o", out,
                           os.path.join(HERE, "sim_change", "sim_change.cpp")])
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    # built into a temporary directory: a read-only checkout passes too
    return build_driver(str(tmp_path_factory.mktemp("sim_change") / "sim_change"))


@pytest.fixture(scope="module")
def mutant_drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("sim_change_mutants")
    return {m: build_driver(str(d / m.lower()), m) for m in cc.MUTANT_CASES}


def run(driver, tmp, b, want_cells=True, want_list=True, items_per_wave=0):
    """-> (prev after, grids or None, summaries, list words or None, count or None); items_per_wave 0: the launcher's choice"""
    inp, outp = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    flags = (1 if want_cells else 0) | (2 if want_list else 0) | (4 if b.words else 0) | items_per_wave << 8
    with open(inp, "wb") as f:
        f.write(struct.pack("<8I", b.w, b.h, b.n, b.cl, b.roll, b.thr, b.min_changed, flags))
        f.write(struct.pack("<9Q", b.cur_off, b.cur_pitch, b.cur_stride, b.cur_buf.size, b.set1, b.prev_off, b.prev_pitch, b.prev_stride,
                            b.prev_buf.size))
        if b.words:
            f.write(np.asarray(b.words, np.uint32).tobytes())
        f.write(b.cur_buf.tobytes())
        f.write(b.prev_buf.tobytes())
    r = subprocess.run([driver, inp, outp], capture_output=True, text=True, env=ENV, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.fromfile(outp, np.uint8)
    at = [0]

    def take(nbytes, dtype):
        out = raw[at[0]:at[0] + nbytes].view(dtype)
        at[0] += nbytes
        return out
    prev = take(b.prev_buf.size, np.uint8)
    cells = take(b.n * b.gw * b.gh * 4, np.uint32).reshape(b.n, b.gh, b.gw) if want_cells else None
    summ = take(b.n * 16, SUMMARY)
    lst = take(b.n * 4, np.uint32) if want_list else None
    count = int(take(4, np.uint32)[0]) if want_list else None
    assert at[0] == raw.size
    return prev, cells, summ, lst, count


def compare(b, got):
    """None, or what differs from the reference"""
    prev, cells, summ, lst, count = got
    grid, want_summ, want_sel, want_prev = cc.expected(b)
    if cells is not None:
        want_cells = np.where(np.asarray(b.valid)[:, None, None], grid, SENTINEL)
        if not (cells == want_cells).all():
            p, cy, cx = [int(v[0]) for v in np.nonzero(cells != want_cells)]
            return "cell (%d, %d, %d): %#x, want %#x" % (p, cy, cx, cells[p, cy, cx], want_cells[p, cy, cx])
    if [tuple(int(v) for v in s) for s in summ] != want_summ:
        return "summaries %r, want %r" % (summ.tolist(), want_summ)
    if lst is not None:
        if count != len(want_sel) or lst[:count].tolist() != want_sel:
            return "list %r (%r), want %r" % (lst[:min(count, b.n)].tolist(), count, want_sel)
        if not (lst[count:] == SENTINEL).all():
            return "entries behind the count were written"
    if not (prev == want_prev).all():
        return "prev differs at byte %d" % int(np.nonzero(prev != want_prev)[0][0])
    return None


def test_every_hazard_occurs_among_the_cases():
    cc.check_hazards()


@pytest.mark.parametrize("name", list(cc.CASES))
def test_cases_lane_by_lane(driver, tmp_path, name):
    b = cc.build(name)
    assert compare(b, run(driver, str(tmp_path), b)) is None


@pytest.mark.parametrize("items_per_wave", [2, 3, 16])
@pytest.mark.parametrize("name", ["size_2049x8_c8", "size_1025x9_c8", "size_176x144_c8", "size_33x65_c8", "corners_c16", "segment_c32",
                                  "words_invalid_and_sets", "extreme_c64_wide", "height_c8+1"])
def test_a_wave_that_takes_several_items(driver, tmp_path, name, items_per_wave):
    """the launcher gives a wave several items only in launches of thousands (many_items_*): here every small shape gets them"""
    b = cc.build(name)
    assert b.gh * -(-b.w // cc.SEG) > 1
    assert compare(b, run(driver, str(tmp_path), b, items_per_wave=items_per_wave)) is None


@pytest.mark.parametrize("name", ["size_1025x9_c8", "corners_c32", "words_invalid_and_sets", "select_n130_roll"])
def test_without_a_grid_and_without_a_list(driver, tmp_path, name):
    b = cc.build(name)
    assert compare(b, run(driver, str(tmp_path), b, want_cells=False, want_list=False)) is None


@pytest.mark.parametrize("mutant", list(cc.MUTANT_CASES))
def test_a_mutant_fails_its_named_cases(mutant_drivers, tmp_path, mutant):
    for name in cc.MUTANT_CASES[mutant]:
        b = cc.build(name)
        assert compare(b, run(mutant_drivers[mutant], str(tmp_path), b)) is not None, name
