"""k_tracks and k_tracks_pack (tracks_picture, tracks_pack: h263-rs_amd/csrc/tracks_kernel.inl) run thread by thread on the CPU under
AddressSanitizer + UBSan (tests/sim_tracks/sim_tracks.cpp: a stand-alone program, run as a child process), against the sequential
reference (tracks_ref), exactly.  The table, the infos, the cut list, the state and every output are heap buffers of exactly their
extents: ASan sees any access outside, and inside them every byte is compared after EVERY call of a sequence -- the state, the
invalid tail of the table and the zero refs behind the count too.  The cases are tracks_cases.CASES; that each hazard occurs among
them is asserted on the reference's side.  The three mutants of mutants.h must fail the cases named for them."""
import os
import struct
import subprocess

import numpy as np
import pytest

import tracks_cases as tc
import tracks_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")


def build_driver(out, *defines):
    subprocess.check_call(["g++", "-O1", "-g", "-fno-strict-aliasing", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *["-D" + d for d in defines], "-o", out,
                           os.path.join(HERE, "sim_tracks", "sim_tracks.cpp")])
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    # built into a temporary directory: a read-only checkout passes too
    return build_driver(str(tmp_path_factory.mktemp("sim_tracks") / "sim_tracks"))


@pytest.fixture(scope="module")
def mutant_drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("sim_tracks_mutants")
    return {m: build_driver(str(d / m.lower()), m) for m in tc.MUTANT_CASES}


def run(driver, tmp, k, order=0):
    """-> per call (state, rois, refs or None, info, count) as the launches left them"""
    inp, outp = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    p = k.prm
    with open(inp, "wb") as f:
        f.write(struct.pack("<12I", k.w, k.h, k.n, p.max_tracks, p.iou_permille, p.max_missed, p.min_hits, p.emit_period, k.max_out,
                            1 if k.refs else 0, order, len(k.calls)))
        f.write(k.state0.tobytes())
        for c in k.calls:
            has_cut = c.cut is not None
            f.write(struct.pack("<4I", c.rois.size, int(has_cut), c.cut.size if has_cut else 0, c.cut_count if has_cut else 0))
            f.write(c.rois.tobytes())
            f.write(c.info_in.tobytes())
            if has_cut:
                f.write(c.cut.tobytes())
    r = subprocess.run([driver, inp, outp], capture_output=True, text=True, env=ENV, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.fromfile(outp, np.uint8)
    at = [0]

    def take(nbytes, dtype):
        out = raw[at[0]:at[0] + nbytes].view(dtype)
        at[0] += nbytes
        return out
    calls = []
    for _ in k.calls:
        state = take(k.state_bytes, np.uint8)
        rois = take(k.max_out * 16, ref.ROI)
        refs = take(k.max_out * 16, ref.REF) if k.refs else None
        info = take(k.n * 32, ref.INFO)
        calls.append((state, rois, refs, info, take(8, np.uint32)))
    assert at[0] == raw.size
    return calls


def first_difference(name, got):
    for c, (want, g) in enumerate(zip(tc.expected(name), got)):
        d = tc.compare(want, *g)
        if d is not None:
            return "call %d: %s" % (c, d)
    return None


def test_every_hazard_occurs_among_the_cases():
    tc.check_hazards()


@pytest.mark.parametrize("name", list(tc.CASES))
def test_cases_thread_by_thread(driver, tmp_path, name):
    assert first_difference(name, run(driver, str(tmp_path), tc.build(name))) is None


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name", tc.MULTI_ROUND)
def test_the_threads_of_a_phase_in_another_order(driver, tmp_path, name, order):
    """the device runs a phase's threads in any order: descending and scattered give the same bytes"""
    assert first_difference(name, run(driver, str(tmp_path), tc.build(name), order)) is None


@pytest.mark.parametrize("mutant", list(tc.MUTANT_CASES))
def test_a_mutant_fails_its_named_cases(mutant_drivers, tmp_path, mutant):
    for name in tc.MUTANT_CASES[mutant]:
        assert first_difference(name, run(mutant_drivers[mutant], str(tmp_path), tc.build(name))) is not None, name
