"""The bookkeeping of the reconstruction waves -- record forms, fill, wave kinds, group words -- on the CPU.

For every picture of the designed tables of tests/wave_cases.py:
  * the C oracle and the kernel phases compiled for the CPU (tests/sim/sim.cpp) agree on every plane byte, with dense
    coefficient blocks and with events, and for P pictures also with sparse records (group words);
  * what the checker's hand-written wave driver DECIDED per wave (sim_wave_stats: n_active, static, MC, all_inter, the group
    word, the form of every round) equals the anatomy that wave_cases restates from the design -- so the driver takes the
    paths the design says the device takes, the dense-round instantiations among them;
  * every signature block changes pixels when the coefficient pool is shifted by one slot either way, and no signature
    residual is hidden by the final clamp;
  * the classifier finds nothing of the table's declared case space missing.
The three mutants of the bookkeeping (csrc/mutants.h), built into the checker, must equal their record-editing models byte
for byte -- the same assertion tests/test_gpu_mutation.py makes of the gfx950 builds."""
import numpy as np
import pytest

import simlib
import wave_cases as wc
from oracle import oracle as orc

_REFS = {}
FORM_CODE = {wc.GENERAL: simlib.ROUND_GENERAL, wc.DENSE: simlib.ROUND_DENSE, wc.WIDE: simlib.ROUND_WIDE}


def reference(w, h, records=None):
    key = (w, h, records is not None)
    if key not in _REFS:
        mbs, co = records or wc.reference_records(w, h)
        rc, planes = orc.decode_picture(w, h, mbs, co, None)
        assert rc == 0
        lo, hi = min(int(p.min()) for p in planes), max(int(p.max()) for p in planes)
        assert 64 <= lo and hi <= 191, "the key frame must be mid-range: %d..%d" % (lo, hi)
        assert all(np.ptp(v[y:y + 8, x:x + 8]) > 0 for v in wc.plane_views({"w": w, "h": h}, planes)
                   for y in range(0, v.shape[0] - 7, 8) for x in range(0, v.shape[1] - 7, 8)), "... and textured in every block"
        _REFS[key] = planes
    return _REFS[key]


def check_stats(pic, waves, sparse, what):
    """the checker's per-wave report of its last call against the anatomy"""
    stats = {(int(s["mby"]), int(s["group"])): s for s in simlib.wave_stats()}
    assert len(stats) == len(waves), (what, len(stats), len(waves))
    for a in waves:
        s = stats[(a["mby"], a["group"])]
        where = "%s, table (%s) %s, wave (row %d, group %d)" % (what, pic["table"], pic["tag"], a["mby"], a["group"])
        assert int(s["valid"]) == a["valid"], where
        assert int(s["group_word"]) == (a["group_word"] if sparse else 0), where
        if sparse and a["copy_by_word"]:
            assert int(s["is_static"]) == 2, where
            continue
        assert int(s["n_active"]) == a["n_active"], where
        assert int(s["is_static"]) == (1 if a["static"] else 0), where
        if a["static"]:
            continue
        assert (int(s["mc"]), int(s["all_inter"])) == (int(a["mc"]), int(a["all_inter"])), where
        assert int(s["n_rounds"]) == a["n_rounds"], where
        assert [int(f) for f in s["form"][:a["n_rounds"]]] == [FORM_CODE[f] for f in a["forms"]], where


def check_signatures(pic, waves, want, ref):
    """a block read from a neighbouring pool slot changes pixels; no signature residual is hidden by the clamp"""
    regions = wc.signature_regions(pic, waves)
    views = wc.plane_views(pic, want)
    for k, x, y, _ in regions:
        blk = views[k][y:y + 8, x:x + 8]
        assert 1 <= blk.min() and blk.max() <= 254, ("a residual may be hidden by the clamp", pic["table"], pic["tag"], k, x, y)
    if len(pic["coeffs"]) < 2 or not regions:
        return
    for shift in (1, -1):
        rc, moved = orc.decode_picture(pic["w"], pic["h"], pic["mbs"], np.roll(pic["coeffs"], shift, axis=0), ref)
        assert rc == 0
        # (the block at the end of the pool that the shift wraps around to the other end has no designed neighbour)
        wrapped = 0 if shift == 1 else len(pic["coeffs"]) - 1
        missing = {r[:3] for r in regions if r[3] != wrapped} - wc.differing_blocks(pic, moved, want)
        assert not missing, ("the pool shifted by %d leaves blocks unchanged" % shift, pic["table"], pic["tag"], sorted(missing)[:5])


def check_picture(pic, cov, ref=None, signatures=True):
    """oracle == kernel phases in every transport; the driver's decisions == the anatomy; -> the oracle's planes"""
    w, h, mbs, co = pic["w"], pic["h"], pic["mbs"], pic["coeffs"]
    is_p = pic["picture_type"] != wc.PICTURE_I
    if is_p and ref is None:
        ref = reference(w, h)
    rc, want = orc.decode_picture(w, h, mbs, co, ref if is_p else None)
    assert rc == 0
    waves = wc.anatomy(pic)
    sparse_waves = wc.anatomy(pic, sparse=True) if is_p else None
    for events in (False, True):
        for sparse in ((False, True) if is_p else (False,)):
            what = "%s coefficients, %s records" % ("events" if events else "dense", "sparse" if sparse else "dense")
            status, got = simlib.recon(w, h, mbs, co, ref if is_p else None, events=events, sparse_records=sparse)
            assert status == 0, what
            diff = wc.first_difference(pic, got, want, waves)
            assert diff is None, "kernel phases on the CPU, %s: %s" % (what, diff)
            check_stats(pic, sparse_waves if sparse else waves, sparse, what)
    if signatures:
        check_signatures(pic, waves, want, ref if is_p else None)
    cov.add(pic, waves, sparse_waves)
    return want


# ---------------------------------------------------------------------------------------------------------------
def test_table_a_every_record_form_in_p_pictures():
    cov = wc.Coverage()
    for pic in wc.table_a_p():
        check_picture(pic, cov)
    assert cov.missing_a((wc.PICTURE_P,)) == []


def test_table_a_every_intra_record_form_in_i_pictures():
    cov = wc.Coverage()
    for pic in wc.table_a_i():
        check_picture(pic, cov)
    assert cov.missing_a((wc.PICTURE_I,)) == []


def test_table_a_uncoded_intra_blocks_with_the_edge_codes():
    cov = wc.Coverage()
    for pic in wc.table_a_dc():
        check_picture(pic, cov)
    assert cov.missing_a_dc() == []


@pytest.mark.parametrize("kind", wc.B_KINDS)
def test_table_b_every_fill(kind):
    cov = wc.Coverage()
    for pic in wc.table_b((kind,)):
        check_picture(pic, cov)
    assert cov.missing_b((kind,)) == []


def test_table_b_with_every_round_forced_wide():
    """which rounds take the wide form is a matter of speed only: forced, the pictures must not change (and the driver says
    that it took it)"""
    L = simlib.lib()
    L.sim_force_wide_rounds(1)
    try:
        for pic in wc.table_b():
            is_p = pic["picture_type"] != wc.PICTURE_I
            ref = reference(pic["w"], pic["h"]) if is_p else None
            rc, want = orc.decode_picture(pic["w"], pic["h"], pic["mbs"], pic["coeffs"], ref)
            for events in (False, True):
                status, got = simlib.recon(pic["w"], pic["h"], pic["mbs"], pic["coeffs"], ref, events=events)
                assert status == 0
                diff = wc.first_difference(pic, got, want)
                assert diff is None, "every round wide, %s: %s" % ("events" if events else "dense", diff)
                forms = {int(f) for s in simlib.wave_stats() for f in s["form"][:int(s["n_rounds"])]}
                assert forms <= {simlib.ROUND_WIDE}
    finally:
        L.sim_force_wide_rounds(0)


def test_table_c_wave_kinds_and_widths():
    cov = wc.Coverage()
    for pic in wc.table_c():
        check_picture(pic, cov)
    assert cov.missing_c() == []


@pytest.mark.parametrize("n", range(1, 8))
def test_table_d_every_group_word(n):
    """the records of the bitstream table through the checker (its sparse transport makes the group words), and what the
    host parser makes of their bitstreams: the same records"""
    import parselib as pl
    import sorenson_enc as enc
    from test_bitstream_e2e import assert_records_equal
    w, h = wc.d_size(n)
    ref = reference(w, h, wc.d_reference_records(n))
    cov = wc.Coverage()
    for pic in wc.table_d((n,)):
        check_picture(pic, cov, ref)
        rc, d, got, gco, _ = pl.parse_picture(enc.encode_picture(w, h, 1, wc.D_PQUANT, pic["mbs"], pic["coeffs"], temporal_reference=1))
        assert rc == 0 and (d.width, d.height, d.picture_type) == (w, h, 1)
        assert_records_equal(got, pic["mbs"])
        assert (gco == pic["coeffs"]).all()
    assert cov.missing_d((n,)) == []


def test_the_dense_i_picture_takes_the_dense_instantiations():
    """the synthetic dense I picture (every block Full, every row reaching its last pair): every full round of every wave is
    a dense round, and the dense instantiations give the oracle's bytes"""
    w, h = 176, 144
    mbs, co = simlib.synth_picture(0, w, h, 3, 0)
    rc, want = orc.decode_picture(w, h, mbs, co, None)
    assert rc == 0
    for events in (False, True):
        status, got = simlib.recon(w, h, mbs, co, events=events)
        assert status == 0 and all((g == e).all() for g, e in zip(got, want))
        stats = simlib.wave_stats()
        assert len(stats) == 9 * 2
        for s in stats:
            # every round of eight blocks is a dense round; the right-edge wave (3 macroblocks, 18 blocks) ends in a round of two
            n = int(s["n_active"])
            assert n == 6 * bin(int(s["valid"])).count("1") and int(s["n_rounds"]) == (n + 7) // 8
            assert [int(f) for f in s["form"][:n // 8]] == [simlib.ROUND_DENSE] * (n // 8)
            assert [int(f) for f in s["form"][n // 8:int(s["n_rounds"])]] == [simlib.ROUND_GENERAL] * (n % 8 != 0)


def test_the_coverage_notices_a_missing_case():
    """the zero-missing conditions are not vacuous"""
    cov = wc.Coverage()
    pics = list(wc.table_b(("mixed",)))
    for pic in pics[1:]:
        cov.add(pic)
    assert cov.missing_b(("mixed",)) != []
    cov.add(pics[0])
    assert cov.missing_b(("mixed",)) == []
    cov = wc.Coverage()
    for pic in wc.table_c():
        if pic["tag"]["kind"] != "near":
            cov.add(pic)
    assert ("near static at width", 8) in cov.missing_c() and ("right edge, near static", 7, 6) in cov.missing_c()


# ---------------------------------------------------------------------------------------------------------------
# the mutants
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", ["killkeep", "staticmv", "intradc"])
def test_mutation_models_predict_the_mutant_checker_builds(mutant):
    import wave_mutation_probe as probe
    product = probe.expectations()
    model = probe.expectations(mutant)
    for (name, pic, want), (_, _, predicted) in zip(product, model):
        ref = probe.reference(pic)
        status, got = simlib.recon(pic["w"], pic["h"], pic["mbs"], pic["coeffs"], ref)
        assert status == 0 and wc.first_difference(pic, got, want) is None, "the product checker is clean on the probe"
        status, got = simlib.recon(pic["w"], pic["h"], pic["mbs"], pic["coeffs"], ref, variant=mutant)
        diff = wc.first_difference(pic, got, predicted)
        assert diff is None, "the %s mutant (got) against its model (expected), picture %s: %s" % (mutant, name, diff)
        where = wc.differing_blocks(pic, predicted, want)
        assert where, "the %s model does not differ from the product on picture %s" % (mutant, name)
        stray = where - probe.predicted_blocks(pic, mutant)
        assert not stray, "the %s model differs outside the blocks the anatomy names, picture %s: %s" % (mutant, name, sorted(stray)[:5])
