"""Motion compensation swept over every vector phase, border and width -- on the CPU.

Three implementations must agree on every plane byte of the designed tables of tests/mc_cases.py:
  the C oracle (oracle/h263_oracle.c), the independent numpy restatement (oracle/np_restatement.py; its whole-plane form
  where nothing is coded, its per-macroblock loop else) and the kernel phases themselves, compiled for the CPU
  (tests/sim/sim.cpp) -- the latter once with dense and once with sparse records.
Every test also asserts that the classifier of mc_cases finds NOTHING of the table's declared case space missing: a
case that the builders stopped producing fails the test like a wrong pixel does.

The reference picture of a case is the oracle's decode of mc_cases.reference_records (a key frame): the GPU twin of
this file (test_gpu_mc_sweep.py) can install the same one.  Table (f) is the exception here: the CPU implementations
take any planes as their reference, so they get the 528 x 528 construction itself."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mc_cases as mc
import simlib
from oracle import np_restatement as npr
from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
_REFS = {}


def reference(w, h):
    if (w, h) not in _REFS:
        mbs, co = mc.reference_records(w, h)
        rc, planes = orc.decode_picture(w, h, mbs, co, None)
        assert rc == 0
        _REFS[(w, h)] = planes
    return _REFS[(w, h)]


def three_way(pic, ref=None, asan=False, transports=(False, True)):
    """oracle == numpy restatement == kernel phases (dense records, sparse records) on every byte"""
    w, h, mbs, co = pic["w"], pic["h"], pic["mbs"], pic["coeffs"]
    ref = reference(w, h) if ref is None else ref
    rc, want = orc.decode_picture(w, h, mbs, co, ref)
    assert rc == 0
    try:
        rc, restated = npr.predict_picture(w, h, mbs, ref)
    except ValueError:
        rc, restated = npr.decode_picture(w, h, mbs, co, ref)
    assert rc == 0
    diff = mc.first_difference(pic, restated, want)
    assert diff is None, "numpy restatement (got) against the C oracle (expected): " + diff
    for sparse in transports:
        status, got = simlib.recon(w, h, mbs, co, ref, sparse_records=sparse, asan=asan)
        assert status == 0
        diff = mc.first_difference(pic, got, want)
        assert diff is None, "kernel phases on the CPU, %s records: %s" % ("sparse" if sparse else "dense", diff)
    return want


def integer_waves():
    out = (C.c_uint64 * 2)()
    simlib.lib().sim_integer_waves(out)
    return int(out[0]), int(out[1])


# ---------------------------------------------------------------------------------------------------------------
A_GROUPS = [tuple(range(1, 41)), tuple(range(41, 81)), (128,), (1920,)]


@pytest.mark.parametrize("widths", A_GROUPS, ids=["1-40", "41-80", "128", "1920"])
def test_table_a_every_width_block_column_window_start_and_phase(widths):
    cov = mc.Coverage()
    for pic in mc.table_a(widths):
        three_way(pic)
        cov.add(pic)
    assert cov.missing_a(widths) == []


def test_table_b_every_height_row_group_and_row_start():
    cov = mc.Coverage()
    for pic in mc.table_b():
        three_way(pic)
        cov.add(pic)
    assert cov.missing_b() == []


def test_table_c_corners():
    cov = mc.Coverage()
    for pic in mc.table_c():
        three_way(pic)
        cov.add(pic)
    assert cov.missing_c() == []


@pytest.mark.parametrize("short_cut", [True, False], ids=["short_cut_taken", "short_cut_forced_off"])
def test_table_d_whole_wave_integer_vectors(short_cut):
    """the kernel's branch for a wave whose 64 lanes all carry integer vectors, which the CPU checker takes exactly where
    the device does (sim.cpp makes the two ballots); forced off, the general form must give the same pixels"""
    L = simlib.lib()
    cov = mc.Coverage()
    before = integer_waves()
    L.sim_no_integer_short_cut(0 if short_cut else 1)
    try:
        for pic in mc.table_d():
            three_way(pic)
            cov.add(pic)
    finally:
        L.sim_no_integer_short_cut(0)
    taken = tuple(b - a for a, b in zip(before, integer_waves()))
    assert cov.missing_d() == []
    if short_cut:
        assert taken[0] > 100 and taken[1] > 100, taken
    else:
        assert taken == (0, 0)


def test_table_e_every_chroma_vector_sum():
    cov = mc.Coverage()
    for pic in mc.table_e():
        three_way(pic)
        cov.add(pic)
    assert cov.missing_e() == []
    assert len(mc.e_declared(mc.E_WIDTH // 16, mc.E_WIDTH // 2)) > 30000


def test_table_e_wrap_sums_that_leave_the_i16_range():
    """gather.rs:182 adds the four vectors as i16 (h263_oracle.c:387-390, "i16 adds"): a RELEASE build of the reference
    wraps, a dev build panics -- the same release-build reading the project takes for the dequantiser's wrap
    (tests/test_dequant_i16_wrap.py).  Four vectors near +-16384 whose true sum is +-65536 + s give the chroma vector of s:
    the chroma block stays inside the picture while every luma tap clamps to its edge.  No host entry point looks at the
    vectors, so nothing refuses such records."""
    cov = mc.Coverage()
    for pic in mc.table_e_wrap():
        three_way(pic)
        cov.add(pic)
    assert cov.missing_e_wrap() == []


def test_table_f_every_pair_of_tap_sums():
    """blend_rows' rounding identity depends on the two tap sums of a pixel alone: all 511 x 511 pairs in one picture"""
    ref = mc.f_reference_planes()
    y = ref[0].reshape(mc.F_LUMA, mc.F_LUMA)
    assert mc.pair_coverage(y).sum() == 511 * 511 == 261121     # (+1/2, +1/2): every pair
    hs, vs = mc.sum_coverage(y)
    assert hs.all() and vs.all()                                # x only, y only: every sum
    for c in ref[1:]:
        # the same construction at 264 x 264 has 263 x 263 positions: (nearly) all of them different pairs, every horizontal sum
        c = c.reshape(mc.F_CHROMA, mc.F_CHROMA)
        assert mc.pair_coverage(c).sum() >= 0.999 * 263 * 263
        assert mc.sum_coverage(c)[0].all()
    for pic in mc.table_f():
        three_way(pic, ref)


def test_table_f_as_flat_blocks_is_decodable_and_keeps_every_pair():
    """what the GPU twin installs: the same samples as flat 8x8 blocks, reached by an INTRADC picture and one push"""
    w, h, intra, push, co = mc.f_blocks_reference()
    rc, planes = orc.decode_picture(w, h, intra, mc.NO_COEFFS, None)
    assert rc == 0
    rc, planes = orc.decode_picture(w, h, push, co, planes)
    assert rc == 0
    want = mc.f_reference_planes()
    for got, e, n in zip(planes, want, (mc.F_LUMA, mc.F_CHROMA, mc.F_CHROMA)):
        g = got.reshape(8 * n, 8 * n)
        assert (g == np.kron(e.reshape(n, n), np.ones((8, 8), np.uint8))).all()
    assert mc.pair_coverage(planes[0].reshape(h, w)).all()


@pytest.mark.parametrize("mutant", ["blend", "intborder"])
def test_mutation_models_predict_the_mutant_checker_builds(mutant):
    """The two motion-compensation mutants of csrc/mutants.h, built into the CPU checker: on the probe pictures of
    tests/mc_mutation_probe.py (tables (d) and (f), the latter as flat blocks) each must differ from the oracle and equal
    its numpy model on every byte -- the same assertion tests/test_gpu_mutation.py makes of the gfx950 builds."""
    import mc_mutation_probe as probe
    w, h, intra, push, co = mc.f_blocks_reference()
    rc, f_ref = orc.decode_picture(w, h, intra, mc.NO_COEFFS, None)
    rc, f_ref = orc.decode_picture(w, h, push, co, f_ref)
    differing = {"d": 0, "f": 0}
    for table, pics in (("d", probe.pictures_d()), ("f", probe.pictures_f())):
        for pic in pics:
            ref = f_ref if table == "f" else reference(pic["w"], pic["h"])
            rc, want = orc.decode_picture(pic["w"], pic["h"], pic["mbs"], pic["coeffs"], ref)
            model = (probe.model_blend if mutant == "blend" else probe.model_intborder)(pic, ref, want)
            status, got = simlib.recon(pic["w"], pic["h"], pic["mbs"], pic["coeffs"], ref, variant=mutant)
            diff = mc.first_difference(pic, got, model)
            assert diff is None, "the %s mutant (got) against its model (expected): %s" % (mutant, diff)
            differing[table] += mc.first_difference(pic, got, want) is not None
    print(mutant, "pictures that differ from the oracle:", differing)
    assert differing["f" if mutant == "blend" else "d"] > 0


def test_the_classifier_notices_a_missing_case():
    """the zero-missing condition is not vacuous: drop one picture of a table and the classifier names what went"""
    cov = mc.Coverage()
    pics = list(mc.table_a((24,)))
    for pic in pics[1:]:
        cov.add(pic)
    assert cov.missing_a((24,)) != []
    cov.add(pics[0])
    assert cov.missing_a((24,)) == []
    cov = mc.Coverage()
    for pic in mc.table_d((128, 176)):
        if not pic["tag"].get("intra"):
            cov.add(pic)
    assert ("Y", "intra") in cov.missing_d() and ("C", "intra") in cov.missing_d()


def test_tables_a_to_d_under_asan_and_ubsan():
    """the kernel phases under AddressSanitizer + UBSan (child process, libasan preloaded) on tables (a)-(d): every
    "the 12-byte load may run past the row end" of the fetch phase, at every width"""
    asan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"]).decode().strip()
    subprocess.check_call(["make", "-C", simlib.SIM_DIR, "-s", "libh263mi_sim_asan.so"])    # (built here, not under the preload)
    code = (
        "import sys; sys.path[:0]=[%r,%r]\n"
        "import mc_cases as mc, test_sim_mc_sweep as t\n"
        "n = 0\n"
        "for table in (mc.table_a, mc.table_b, mc.table_c, mc.table_d):\n"
        "    for pic in table():\n"
        "        t.three_way(pic, asan=True, transports=(n %% 2 == 1,))\n"
        "        n += 1\n"
        "print('asan-ok', n)\n" % (os.path.dirname(HERE), HERE))
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=3000)
    assert out.returncode == 0 and "asan-ok" in out.stdout, out.stderr[-3000:]
