"""k_hist, k_hist_final and k_hist_select (hist_wave, hist_final, hist_select: h263-rs_amd/csrc/hist_kernel.inl) run lane by lane on
the CPU under AddressSanitizer + UBSan (tests/sim_hist/sim_hist.cpp: a stand-alone program, run as a child process), against the
numpy reference (hist_ref), exactly.  The planes are a heap buffer of exactly the set's bytes, the histograms, prev, the statistics
and the list buffers of exactly their extents: ASan sees any access outside.  The cases are hist_cases.CASES; that each hazard
occurs among them is asserted on the reference's side.  The two mutants of mutants.h must fail the cases named for them."""
import os
import struct
import subprocess

import numpy as np
import pytest

import h263mi
import hist_cases as hc

HERE = os.path.dirname(os.path.abspath(__file__))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")


def build_driver(out, *defines):
    subprocess.check_call(["g++", "-O1", "-g", "-fno-strict-aliasing", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *["-D" + d for d in defines], "-o", out,
                           os.path.join(HERE, "sim_hist", "sim_hist.cpp")])
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    # built into a temporary directory: a read-only checkout passes too
    return build_driver(str(tmp_path_factory.mktemp("sim_hist") / "sim_hist"))


@pytest.fixture(scope="module")
def mutant_drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("sim_hist_mutants")
    return {m: build_driver(str(d / m.lower()), m) for m in hc.MUTANT_CASES}


def run(driver, tmp, b, want_list=None, items_per_wave=0, prev="case"):
    """-> (hist, prev after or None, stats, list words or None, count or None); items_per_wave 0: the launcher's choice; prev: the
    case's, or an (n, 256) array in its place"""
    prev = b.prev if isinstance(prev, str) else prev
    want_list = (prev is not None) if want_list is None else want_list
    inp, outp = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    flags = (1 if prev is not None else 0) | (2 if want_list else 0) | (4 if b.words else 0)
    with open(inp, "wb") as f:
        f.write(struct.pack("<12I", b.w, b.h, b.n, b.roll, b.lo, b.hi, b.cut, flags, items_per_wave, 0, 0, 0))
        f.write(struct.pack("<5Q", b.off, b.pitch, b.stride, b.buf.size, b.set1))
        if b.words:
            f.write(np.asarray(b.words, np.uint32).tobytes())
        f.write(b.buf.tobytes())
        if prev is not None:
            f.write(np.ascontiguousarray(prev, np.uint32).tobytes())
    r = subprocess.run([driver, inp, outp], capture_output=True, text=True, env=ENV, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.fromfile(outp, np.uint8)
    at = [0]

    def take(nbytes, dtype):
        out = raw[at[0]:at[0] + nbytes].view(dtype)
        at[0] += nbytes
        return out
    hist = take(b.n * 1024, np.uint32).reshape(b.n, 256)
    after = take(b.n * 1024, np.uint32).reshape(b.n, 256) if prev is not None else None
    stats = take(b.n * 32, h263mi.HIST_STATS_DTYPE)
    lst = take(b.n * 4, np.uint32) if want_list else None
    count = int(take(4, np.uint32)[0]) if want_list else None
    assert at[0] == raw.size
    return hist, after, stats, lst, count


def check(b, got):
    hist, after, stats, lst, count = got
    return hc.compare(b, hist, after, stats, lst, count)


def test_every_hazard_occurs_among_the_cases():
    hc.check_hazards()


@pytest.mark.parametrize("name", list(hc.CASES))
def test_cases_lane_by_lane(driver, tmp_path, name):
    b = hc.build(name)
    assert check(b, run(driver, str(tmp_path), b)) is None


@pytest.mark.parametrize("items_per_wave", [2, 3, 16])
@pytest.mark.parametrize("name", ["size_2049x17", "size_1025x9", "size_17x17", "size_1x2", "place_1_plus1_padded_w100", "decoded", "flat_255",
                                  "words_invalid_and_sets", "overlap_rows", "select_n65"])
def test_a_wave_that_takes_several_items(driver, tmp_path, name, items_per_wave):
    """the launcher gives a wave several items only in launches of thousands (many_items_*): here every small shape gets them"""
    b = hc.build(name)
    assert check(b, run(driver, str(tmp_path), b, items_per_wave=items_per_wave)) is None


@pytest.mark.parametrize("name", ["size_1025x9", "cut_equal_and_above", "words_invalid_and_sets", "select_n130", "prev_ones"])
def test_with_prev_but_without_a_list(driver, tmp_path, name):
    b = hc.build(name)
    assert check(b, run(driver, str(tmp_path), b, want_list=False)) is None


def test_a_second_call_after_a_roll(driver, tmp_path):
    """the prev that a rolling call leaves is the first call's histograms: the same pictures again are at distance 0 and no cuts,
    other pictures at the distance of the two calls' histograms"""
    first, other = hc.build("cut_first_call"), hc.build("pctl_exact")
    assert first.roll and (first.w, first.h, first.n) == (other.w, other.h, other.n)
    hist, after, stats, lst, count = run(driver, str(tmp_path), first)
    assert check(first, (hist, after, stats, lst, count)) is None and count == 2
    hist2, after2, stats2, lst2, count2 = run(driver, str(tmp_path), first, prev=after)
    assert (hist2 == hist).all() and (after2 == hist).all() and count2 == 0 and not stats2["distance"].any()
    assert (stats2["sum"] == stats["sum"]).all()
    hist3, after3, stats3, _, _ = run(driver, str(tmp_path), other, prev=after)
    want = [hc.ref.distance(other.hist[p], first.hist[p]) for p in range(other.n)]
    assert stats3["distance"].tolist() == want and min(want) > 0
    assert (after3 == after).all()                               # (roll off: prev is an anchor)


@pytest.mark.parametrize("mutant", list(hc.MUTANT_CASES))
def test_a_mutant_fails_its_named_cases(mutant_drivers, tmp_path, mutant):
    for name in hc.MUTANT_CASES[mutant]:
        b = hc.build(name)
        assert check(b, run(mutant_drivers[mutant], str(tmp_path), b)) is not None, name
