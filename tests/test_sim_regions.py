"""k_regions and k_regions_pack (regions_picture, regions_pack: h263-rs_amd/csrc/regions_kernel.inl) run thread by thread on the CPU under
AddressSanitizer + UBSan (tests/sim_regions/sim_regions.cpp: a stand-alone program, run as a child process), against the flood-fill
reference (regions_ref), exactly.  The grids, the staging area, the table, the stats, the info and the counts are heap buffers of
exactly their extents: ASan sees any access outside, and inside them every byte is compared, the invalid tail of the table too.  The
cases are regions_cases.CASES; that each hazard occurs among them is asserted on the reference's side.  The two mutants of mutants.h
must fail the cases named for them."""
import os
import struct
import subprocess

import numpy as np
import pytest

import regions_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")


def build_driver(out, *defines):
    subprocess.check_call(["g++", "-O1", "-g", "-fno-strict-aliasing", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *["-D" + d for d in defines], "-o", out,
                           os.path.join(HERE, "sim_regions", "sim_regions.cpp")])
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    # built into a temporary directory: a read-only checkout passes too
    return build_driver(str(tmp_path_factory.mktemp("sim_regions") / "sim_regions"))


@pytest.fixture(scope="module")
def mutant_drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("sim_regions_mutants")
    return {m: build_driver(str(d / m.lower()), m) for m in rc.MUTANT_CASES}


def run(driver, tmp, k, order=0):
    """-> (rois, stats or None, info, count) as the launch left them"""
    inp, outp = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    flags = (1 if k.summary is not None else 0) | (2 if k.stats else 0)
    with open(inp, "wb") as f:
        f.write(struct.pack("<12I", k.w, k.h, k.n, k.cl, k.conn, k.margin, k.thr, k.min_cells, k.max_per, k.max_rois, flags, order))
        if k.summary is not None:
            f.write(np.array(k.summaries(), dtype=rc.SUMMARY).tobytes())
        f.write(k.grids.tobytes())
    r = subprocess.run([driver, inp, outp], capture_output=True, text=True, env=ENV, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.fromfile(outp, np.uint8)
    at = [0]

    def take(nbytes, dtype):
        out = raw[at[0]:at[0] + nbytes].view(dtype)
        at[0] += nbytes
        return out
    rois = take(k.max_rois * 16, rc.ROI)
    stats = take(k.max_rois * 16, rc.STAT) if k.stats else None
    info = take(k.n * 16, rc.INFO)
    count = take(8, np.uint32)
    assert at[0] == raw.size
    return rois, stats, info, count


def test_every_hazard_occurs_among_the_cases():
    rc.check_hazards()


@pytest.mark.parametrize("name", list(rc.CASES))
def test_cases_thread_by_thread(driver, tmp_path, name):
    k = rc.build(name)
    assert rc.compare(k, *run(driver, str(tmp_path), k)) is None


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name", ["grid_63_c8", "grid_65_c4", "cap_256x128_c4", "cap_256x128_c8", "cap_8192x4", "cap_4x8192", "checkerboard_cap_c8",
                                  "serpentine_cap", "serpentine_tall", "spiral_cap", "comb", "comb_upside_down", "two_us", "pictures_130"])
def test_the_threads_of_a_phase_in_another_order(driver, tmp_path, name, order):
    """the device runs a phase's threads in any order: descending and scattered give the same bytes"""
    k = rc.build(name)
    assert rc.compare(k, *run(driver, str(tmp_path), k, order)) is None


@pytest.mark.parametrize("mutant", list(rc.MUTANT_CASES))
def test_a_mutant_fails_its_named_cases(mutant_drivers, tmp_path, mutant):
    for name in rc.MUTANT_CASES[mutant]:
        k = rc.build(name)
        assert rc.compare(k, *run(mutant_drivers[mutant], str(tmp_path), k)) is not None, name
