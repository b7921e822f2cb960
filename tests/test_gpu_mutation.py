"""Proof that the GPU parity suite DETECTS an FMA-contracted or re-associated IDCT.

Two mutants of the product library are built from the same sources (h263-rs_amd/Makefile `mutants`):
  libh263mi_fma.so       -ffp-contract=fast instead of off: the compiler fuses the IDCT's multiplies into its adds
  libh263mi_pairwise.so  -DH263MI_MUTATE_PAIRWISE: idct_1d sums its eight products as a balanced tree
On the committed block set (found with the FPU-free soft-float model, tools/find_sensitive_blocks.py) the real
library must reproduce the reference arithmetic (idct.rs:52-65, 171-196) pixel for pixel, and each mutant must NOT.

Two more mutants are of the MOTION COMPENSATION (csrc/mutants.h; probe and models: tests/mc_mutation_probe.py):
  libh263mi_blend.so      blend_rows without its `^ (both & dm)` exclusion: +1 in some pixels of (1/2, 1/2) pieces
  libh263mi_intborder.so  border lanes of an all-integer wave skip the clamped re-gather
Their arithmetic is integer: each must differ from the oracle AND equal its numpy model on every byte.

Three more are of the DEBLOCKING POST-FILTER (csrc/mutants.h; probe and models: tests/post_mutation_probe.py):
  libh263mi_dbhalf.so     |d1 / 2| rounds toward zero where the reference shifts a negative d1
  libh263mi_dbfloor.so    the scalar tails of the reference divide with shifts like its SIMD lanes
  libh263mi_dbwrap.so     the columns that ride in the last post tile miss the horizontal block edges
Likewise: each differs from the oracle and equals, on every byte, the numpy restatement with that mutation switched on.

Three more are of the BOOKKEEPING of the reconstruction waves (csrc/mutants.h; probe and models: tests/wave_mutation_probe.py):
  libh263mi_killkeep.so   the mark phase ignores the kill bits
  libh263mi_staticmv.so   eight uncoded inter macroblocks are copied from the reference whatever their vectors are
  libh263mi_intradc.so    uncoded blocks of intra macroblocks are not activated
Each has an exact model -- the oracle over edited records -- and must equal it on every byte, through k_recon and k_frame.

The first two, fma and pairwise, are asked again PER FORM of a reconstruction round (tests/idct_form_cases.py; probe:
tests/idct_form_probe.py): the first general round, the later ones, dense rounds and wide rounds, through k_recon and k_frame."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import h263mi
import mutation_probe

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "h263-rs_amd")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if h263mi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")


def expected_luma(blocks, key=None):
    """clamp(128 + residual) per fixture block; with key = a mutation name, the residuals that mutation produces on
    the pixels the fixture lists (the other pixels as in the reference arithmetic)"""
    w, h = mutation_probe.picture_size(len(blocks))
    y = np.full((h, w), 128, np.int32)
    for k, b in enumerate(blocks):
        res = np.array(b["residual"], np.int32)
        if key and key in b["detects"]:
            for yy, xx, v in b["detects"][key]:
                res[yy, xx] = v
        px, py = (k % mutation_probe.MB_COLS) * 16, (k // mutation_probe.MB_COLS) * 16
        y[py:py + 8, px:px + 8] += res
    return np.clip(y, 0, 255).astype(np.uint8)


def run_with(lib_path, tmp_path, name):
    out = str(tmp_path / (name + ".npy"))
    env = dict(os.environ, H263MI_LIB=lib_path)
    subprocess.run([sys.executable, os.path.join(HERE, "mutation_probe.py"), out], env=env, check=True, timeout=300)
    return np.load(out)


def test_the_product_library_reproduces_the_reference_arithmetic_on_the_sensitive_blocks():
    blocks = mutation_probe.fixture()
    got = mutation_probe.decode_luma()
    assert (got == expected_luma(blocks)).all()


@pytest.mark.parametrize("mutant", ["fma", "pairwise"])
def test_mutant_build_is_caught(mutant, tmp_path):
    lib = os.path.join(PKG, "mutants", "libh263mi_%s.so" % mutant)
    if not os.path.exists(lib):                                  # normally built by __graft_entry__.build()
        subprocess.check_call(["make", "-C", PKG, "-s", "mutants"])
    blocks = mutation_probe.fixture()
    want = expected_luma(blocks)
    got = run_with(lib, tmp_path, mutant)
    wrong_blocks = 0
    for k in range(len(blocks)):
        px, py = (k % mutation_probe.MB_COLS) * 16, (k // mutation_probe.MB_COLS) * 16
        wrong_blocks += bool((got[py:py + 8, px:px + 8] != want[py:py + 8, px:px + 8]).any())
    listed = sum(mutant in b["detects"] for b in blocks)
    # the comparison the parity tests make (output == oracle) fails on the mutant ...
    assert wrong_blocks >= 10, "the %s mutant went unnoticed (%d blocks differ)" % (mutant, wrong_blocks)
    # ... and it fails where the soft-float model of that mutation said it would
    predicted = expected_luma(blocks, mutant)
    agree = sum(bool((got[(k // 10) * 16:(k // 10) * 16 + 8, (k % 10) * 16:(k % 10) * 16 + 8] ==
                      predicted[(k // 10) * 16:(k // 10) * 16 + 8, (k % 10) * 16:(k % 10) * 16 + 8]).all())
                for k, b in enumerate(blocks) if mutant in b["detects"])
    print("%s mutant: %d blocks differ from the oracle; %d of the %d blocks the model lists match its prediction exactly"
          % (mutant, wrong_blocks, agree, listed))
    assert agree >= listed // 2
    # the same run through the product build (same process-isolated path) is clean
    clean = run_with(os.path.join(PKG, "libh263mi.so"), tmp_path, "product")
    assert (clean == want).all()


def test_dequantiser_mutant_is_caught_by_the_every_level_test():
    """libh263mi_dequant.so: the dequantiser computes 16 x the value with a saturating multiply-add and clears the four
    low bits, which is what turns a saturated 32767 into 16 * 2047 (recon_kernel.inl: dequant_pair_i16); the mutant
    leaves them set.  tests/test_gpu_round3.py::test_every_level_at_every_quantiser_dequantises_like_the_oracle must
    fail on it and pass on the product (both in fresh processes: the library is chosen at import)."""
    lib = os.path.join(PKG, "mutants", "libh263mi_dequant.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", PKG, "-s", "mutants"])
    # (the LEVELs within 9 bits: rounds with a wider LEVEL take the wrapping dequantiser, which this mutant does not touch)
    cmd = [sys.executable, "-m", "pytest", os.path.join(HERE, "test_gpu_round3.py"), "-x", "-q", "-k", "every_level and within_9_bits",
           "-p", "no:cacheprovider"]
    bad = subprocess.run(cmd, env=dict(os.environ, H263MI_LIB=lib), capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "1 failed" in bad.stdout, bad.stdout[-800:]
    good = subprocess.run(cmd, env=dict(os.environ, H263MI_LIB=os.path.join(PKG, "libh263mi.so")), capture_output=True,
                          text=True, timeout=600)
    assert good.returncode == 0 and "1 passed" in good.stdout, good.stdout[-800:]


def test_wrap_mutant_is_caught_by_the_11_bit_level_test():
    """libh263mi_wrap.so: the dequantiser of rounds with LEVELs outside [-512, 511] uses a SATURATING multiply-add, i.e.
    clamps the mathematical product where a release build of the reference clamps the wrapped i16 one (rle.rs:130-133;
    recon_kernel.inl: dequant_pair_wrap) -- round 1-4's behaviour.  The 11-bit LEVEL sweep and the hand-derived known
    answers of tests/test_gpu_round5.py must fail on it and pass on the product (fresh processes: the library is chosen at
    import)."""
    lib = os.path.join(PKG, "mutants", "libh263mi_wrap.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", PKG, "-s", "mutants"])
    for key, n in (("hand_derived", 1), ("every_11_bit and dense", 1)):
        cmd = [sys.executable, "-m", "pytest", os.path.join(HERE, "test_gpu_round5.py"), "-x", "-q", "-k", key,
               "-p", "no:cacheprovider"]
        bad = subprocess.run(cmd, env=dict(os.environ, H263MI_LIB=lib), capture_output=True, text=True, timeout=600)
        assert bad.returncode != 0 and "1 failed" in bad.stdout, bad.stdout[-800:]
        good = subprocess.run(cmd, env=dict(os.environ, H263MI_LIB=os.path.join(PKG, "libh263mi.so")), capture_output=True,
                              text=True, timeout=600)
        assert good.returncode == 0 and "%d passed" % n in good.stdout, good.stdout[-800:]


# ---------------------------------------------------------------------------------------------------------------
# the motion-compensation mutants
# ---------------------------------------------------------------------------------------------------------------
def _mc_probe(lib_path, tmp_path, name):
    out = str(tmp_path / (name + ".npz"))
    env = dict(os.environ, H263MI_LIB=lib_path)
    subprocess.run([sys.executable, os.path.join(HERE, "mc_mutation_probe.py"), out], env=env, check=True, timeout=900)
    return np.load(out)


@pytest.fixture(scope="module")
def mc_probe_expected():
    """per probe picture: (name, picture, reference planes, the oracle's planes)"""
    import mc_cases as mc
    import mc_mutation_probe as probe
    from oracle import oracle as orc
    out = []
    for k, pic in enumerate(probe.pictures_d()):
        mbs, co = mc.reference_records(pic["w"], pic["h"])
        rc, ref = orc.decode_picture(pic["w"], pic["h"], mbs, co, None)
        rc, want = orc.decode_picture(pic["w"], pic["h"], pic["mbs"], pic["coeffs"], ref)
        assert rc == 0
        out.append(("d%03d" % k, pic, ref, want))
    w, h, intra, push, co = mc.f_blocks_reference()
    rc, ref = orc.decode_picture(w, h, intra, mc.NO_COEFFS, None)
    rc, ref = orc.decode_picture(w, h, push, co, ref)
    for k, pic in enumerate(probe.pictures_f()):
        rc, want = orc.decode_picture(w, h, pic["mbs"], pic["coeffs"], ref)
        assert rc == 0
        out.append(("f%d" % k, pic, ref, want))
    return out


@pytest.mark.parametrize("mutant", ["blend", "intborder"])
def test_mc_mutant_build_fails_exactly_as_its_model_predicts(mutant, tmp_path, mc_probe_expected):
    """tables (d) and (f) of tests/mc_cases.py through a mutant build (child process): it must differ from the oracle, and
    every byte must be the one the numpy model of the mutation predicts (the product build, run the same way, is clean:
    the test below)"""
    import mc_cases as mc
    import mc_mutation_probe as probe
    lib = os.path.join(PKG, "mutants", "libh263mi_%s.so" % mutant)
    if not os.path.exists(lib):                                  # normally built by __graft_entry__.build()
        subprocess.check_call(["make", "-C", PKG, "-s", "mutants"])
    got = _mc_probe(lib, tmp_path, mutant)
    model = probe.model_blend if mutant == "blend" else probe.model_intborder
    differing = {"d": 0, "f": 0}
    wrong_bytes = 0
    for name, pic, ref, want in mc_probe_expected:
        planes = tuple(got["%s_%d" % (name, i)] for i in range(3))
        diff = mc.first_difference(pic, planes, model(pic, ref, want))
        assert diff is None, "the %s mutant (got) against its model (expected), picture %s: %s" % (mutant, name, diff)
        n = sum(int((g != e).sum()) for g, e in zip(planes, want))
        differing[name[0]] += n > 0
        wrong_bytes += n
    print("%s mutant: %d bytes differ from the oracle, in %d pictures of table (d) and %d of table (f); all as its model predicts"
          % (mutant, wrong_bytes, differing["d"], differing["f"]))
    assert differing["f" if mutant == "blend" else "d"] > 0, "the %s mutant went unnoticed" % mutant


def test_mc_probe_through_the_product_build_is_clean(tmp_path, mc_probe_expected):
    """the same child-process path with the product library: every byte is the oracle's"""
    import mc_cases as mc
    clean = _mc_probe(os.path.join(PKG, "libh263mi.so"), tmp_path, "product")
    for name, pic, ref, want in mc_probe_expected:
        diff = mc.first_difference(pic, tuple(clean["%s_%d" % (name, i)] for i in range(3)), want)
        assert diff is None, "the product build, picture %s: %s" % (name, diff)


# ---------------------------------------------------------------------------------------------------------------
# the post-filter mutants
# ---------------------------------------------------------------------------------------------------------------
def _post_probe(lib_path, tmp_path, name):
    out = str(tmp_path / (name + ".npz"))
    env = dict(os.environ, H263MI_LIB=lib_path)
    subprocess.run([sys.executable, os.path.join(HERE, "post_mutation_probe.py"), out], env=env, check=True, timeout=300)
    return np.load(out)


@pytest.fixture(scope="module")
def post_probe_oracle():
    import post_mutation_probe as probe
    return probe.expectations()


@pytest.mark.parametrize("mutant", ["dbhalf", "dbfloor", "dbwrap"])
def test_post_mutant_build_fails_exactly_as_its_model_predicts(mutant, tmp_path, post_probe_oracle):
    """table pictures of tests/post_cases.py through a mutant build (child process): it must differ from the oracle, every
    byte must be the one the numpy model of the mutation predicts, and on the table (a) planes it must differ where the
    classifier says that mutation can show (test_sim_post_sweep.check_where_the_mutant_differs)"""
    import post_mutation_probe as probe
    import test_sim_post_sweep as cpu
    lib = os.path.join(PKG, "mutants", "libh263mi_%s.so" % mutant)
    if not os.path.exists(lib):                                  # normally built by __graft_entry__.build()
        subprocess.check_call(["make", "-C", PKG, "-s", "mutants"])
    got = _post_probe(lib, tmp_path, mutant)
    names, n = probe.compare(got, probe.expectations(mutant))
    assert n == 0, "the %s mutant (got) against its model (expected): %d bytes differ, in %s" % (mutant, n, names[:5])
    names, n = probe.compare(got, post_probe_oracle)
    print("%s mutant: %d bytes differ from the oracle, in %d of %d planes; all as its model predicts" % (mutant, n, len(names), len(post_probe_oracle)))
    assert n > 0, "the %s mutant went unnoticed" % mutant
    cpu.check_where_the_mutant_differs(mutant, got, post_probe_oracle)


def test_post_probe_through_the_product_build_is_clean(tmp_path, post_probe_oracle):
    """the same child-process path with the product library: every byte is the oracle's"""
    import post_mutation_probe as probe
    clean = _post_probe(os.path.join(PKG, "libh263mi.so"), tmp_path, "product")
    names, n = probe.compare(clean, post_probe_oracle)
    assert n == 0, "the product build: %d bytes differ, in %s" % (n, names[:5])


# ---------------------------------------------------------------------------------------------------------------
# the mutants of the reconstruction waves' bookkeeping
# ---------------------------------------------------------------------------------------------------------------
def _wave_probe(lib_path, tmp_path, name):
    out = str(tmp_path / (name + ".npz"))
    env = dict(os.environ, H263MI_LIB=lib_path)
    subprocess.run([sys.executable, os.path.join(HERE, "wave_mutation_probe.py"), out], env=env, check=True, timeout=300)
    return np.load(out)


@pytest.fixture(scope="module")
def wave_probe_oracle():
    import wave_mutation_probe as probe
    return probe.expectations()


@pytest.mark.parametrize("mutant", ["killkeep", "staticmv", "intradc"])
def test_wave_mutant_build_fails_exactly_as_its_model_predicts(mutant, tmp_path, wave_probe_oracle):
    """the probe pictures of tests/wave_mutation_probe.py through a mutant build (child process), by k_recon and by k_frame: every
    byte must be the one the mutation's model -- the oracle over edited records -- predicts, every picture must differ from the
    oracle, and only in the blocks the anatomy names"""
    import wave_cases as wc
    import wave_mutation_probe as probe
    lib = os.path.join(PKG, "mutants", "libh263mi_%s.so" % mutant)
    if not os.path.exists(lib):                                  # normally built by __graft_entry__.build()
        subprocess.check_call(["make", "-C", PKG, "-s", "mutants"])
    got = _wave_probe(lib, tmp_path, mutant)
    wrong = 0
    for (name, pic, want), (_, _, predicted) in zip(wave_probe_oracle, probe.expectations(mutant)):
        for path in ("state", "frame"):
            planes = tuple(got["%s_%s_%d" % (path, name, i)] for i in range(3))
            diff = wc.first_difference(pic, planes, predicted)
            assert diff is None, "the %s mutant (got, %s) against its model (expected), picture %s: %s" % (mutant, path, name, diff)
            where = wc.differing_blocks(pic, planes, want)
            assert where, "the %s mutant went unnoticed on picture %s (%s)" % (mutant, name, path)
            assert where <= probe.predicted_blocks(pic, mutant), (mutant, name, path, sorted(where - probe.predicted_blocks(pic, mutant))[:5])
            wrong += len(where)
    print("%s mutant: %d blocks differ from the oracle; all as its model predicts" % (mutant, wrong))


def test_wave_probe_through_the_product_build_is_clean(tmp_path, wave_probe_oracle):
    """the same child-process path with the product library: every byte is the oracle's"""
    import wave_cases as wc
    clean = _wave_probe(os.path.join(PKG, "libh263mi.so"), tmp_path, "product")
    for name, pic, want in wave_probe_oracle:
        for path in ("state", "frame"):
            diff = wc.first_difference(pic, tuple(clean["%s_%s_%d" % (path, name, i)] for i in range(3)), want)
            assert diff is None, "the product build (%s), picture %s: %s" % (path, name, diff)


# ---------------------------------------------------------------------------------------------------------------
# the arithmetic mutants again, in every form a reconstruction round is compiled in
# ---------------------------------------------------------------------------------------------------------------
def _form_probe(lib_path, tmp_path, name):
    out = str(tmp_path / (name + ".npz"))
    env = dict(os.environ, H263MI_LIB=lib_path)
    subprocess.run([sys.executable, os.path.join(HERE, "idct_form_probe.py"), out], env=env, check=True, timeout=300)
    return np.load(out)


@pytest.fixture(scope="module")
def form_probe_oracle():
    import idct_form_probe as probe
    return probe.expectations()


def _form_detections(got, oracle, mutant):
    """{k_recon / k_frame path: {form name: [listed, differing from the oracle, equal to the model's prediction]}}"""
    import idct_form_probe as probe
    import test_sim_idct_forms as cpu
    return {path: cpu.detections([(pic, want, tuple(got["%s_%s_%d" % (path, name, i)] for i in range(3))) for name, pic, want in oracle], mutant)
            for path in probe.PATHS}


def test_form_probe_through_the_product_build_is_clean(tmp_path, form_probe_oracle):
    """the designed tables of tests/idct_form_cases.py through the child-process path with the product library: every byte is
    the oracle's, through k_recon and k_frame, and every fixture block is its soft-float residual"""
    import idct_form_probe as probe
    import test_sim_idct_forms as cpu
    import wave_cases as wc
    clean = _form_probe(os.path.join(PKG, "libh263mi.so"), tmp_path, "product")
    for name, pic, want in form_probe_oracle:
        for path in probe.PATHS:
            planes = tuple(clean["%s_%s_%d" % (path, name, i)] for i in range(3))
            diff = wc.first_difference(pic, planes, want)
            assert diff is None, "the product build (%s), picture %s: %s" % (path, name, diff)
            cpu.check_fixture_blocks(pic, planes, "the product build (%s)" % path)


def test_pairwise_mutant_is_caught_in_every_form(tmp_path, form_probe_oracle):
    """the pairwise mutation is in the source of idct_1d_pairs, hence in every instantiation: in the first general round, the
    later general rounds, dense rounds and wide rounds, through k_recon and through k_frame, some block the model lists differs
    from the oracle, and at least half of the listed blocks are exactly what the model predicts (the criterion of
    test_mutant_build_is_caught; the CPU checker built with the mutation meets the model on all of them)"""
    import idct_form_cases as fc
    lib = os.path.join(PKG, "mutants", "libh263mi_pairwise.so")
    if not os.path.exists(lib):                                  # normally built by __graft_entry__.build()
        subprocess.check_call(["make", "-C", PKG, "-s", "mutants"])
    counts = _form_detections(_form_probe(lib, tmp_path, "pairwise"), form_probe_oracle, "pairwise")
    for path, forms in counts.items():
        for form in fc.FORM_NAMES:
            listed, differ, agree = forms[form]
            print("pairwise mutant, %s, %s: %d listed placements, %d differ from the oracle, %d equal the model's prediction"
                  % (path, form, listed, differ, agree))
    for path, forms in counts.items():
        for form in fc.FORM_NAMES:
            listed, differ, agree = forms[form]
            assert listed >= 8 and differ >= 1, "the pairwise mutant went unnoticed in %s rounds (%s)" % (form, path)
            assert 2 * agree >= listed, (path, form, listed, agree)


def test_fma_mutant_is_caught_in_the_new_forms(tmp_path, form_probe_oracle):
    """-ffp-contract=fast: WHERE the compiler fuses is its choice, so the counts per form are reported (DESIGN.md section 0, row
    a3) and the assertion is over the union of the forms the designed tables add (later general rounds, dense rounds, wide
    rounds; the first general round has test_mutant_build_is_caught); a form with zero detections says that the
    compiler did not contract there"""
    import idct_form_cases as fc
    lib = os.path.join(PKG, "mutants", "libh263mi_fma.so")
    if not os.path.exists(lib):                                  # normally built by __graft_entry__.build()
        subprocess.check_call(["make", "-C", PKG, "-s", "mutants"])
    counts = _form_detections(_form_probe(lib, tmp_path, "fma"), form_probe_oracle, "fma")
    total = 0
    for path, forms in counts.items():
        for form in fc.FORM_NAMES:
            listed, differ, agree = forms[form]
            print("fma mutant, %s, %s: %d listed placements, %d differ from the oracle, %d equal the model's prediction"
                  % (path, form, listed, differ, agree))
            total += differ if form != "general-first" else 0
    assert total >= 1, "the fma mutant went unnoticed in the later general rounds, the dense rounds and the wide rounds alike"
