"""The arithmetic of the reconstruction rounds in every form it is compiled in, on the CPU (the twin of test_gpu_idct_forms.py).

For every picture of the designed tables of tests/idct_form_cases.py:
  * the C oracle and the kernel phases compiled for the CPU (tests/sim/sim.cpp) agree on every plane byte, with dense
    coefficient blocks and with events, and for P pictures also with sparse records;
  * inside every fixture block the pixels are clamp(base + residual) with the fixture's soft-float residual (base: 128 under a
    P picture, 0 under an I picture);
  * what the checker's wave driver DECIDED (sim_wave_stats: MC, the number of rounds, the form of every round; sim_round_stats:
    n_cols, n_rows, any_special of every round) equals the declaration -- a case that silently takes another form fails here --
    and the declared forms equal the anatomy wave_cases works out from the LEVELs;
  * the classifier finds nothing of the declared case space missing.
The fixture itself (tests/golden/idct_sensitive_forms.json) is held against the C oracle and the soft-float model here too."""
import numpy as np
import pytest

import idct_form_cases as fc
import simlib
import wave_cases as wc
from oracle import oracle as orc
from oracle import softfloat_idct as sf
from test_sim_wave_sweep import FORM_CODE

_WANT = {}


def expected(name, i, pic):
    """the oracle's planes of a picture (computed once)"""
    if (name, i) not in _WANT:
        rc, want = orc.decode_picture(pic["w"], pic["h"], pic["mbs"], pic["coeffs"], fc.flat_reference()[2] if pic["base"] else None)
        assert rc == 0
        _WANT[(name, i)] = want
    return _WANT[(name, i)]


def check_fixture_blocks(pic, planes, what, mutation=None):
    views = wc.plane_views(pic, planes)
    for k, x, y, e, mby, r, slot in pic["placed"]:
        got = views[k][y:y + 8, x:x + 8]
        assert (got == fc.expected_block(e, pic["base"], mutation)).all(), \
            "%s: table (%s) %s, wave %d round %d slot %d: fixture block %s is not clamp(%d + the soft-float residual)" % (
                what, pic["table"], pic["tag"], mby, r, slot, e["id"], pic["base"])


def check_stats(pic, what):
    """the checker's report of its last call against the declaration"""
    stats = {int(s["mby"]): (s, r) for s, r in zip(simlib.wave_stats(), simlib.round_stats())}
    assert len(stats) == len(pic["decl"])
    for mby, d in enumerate(pic["decl"]):
        s, r = stats[mby]
        where = "%s, table (%s) %s, wave %d" % (what, pic["table"], pic["tag"], mby)
        if d["n_active"] == 0 and pic["base"]:
            assert int(s["is_static"]) in (1, 2), where
            continue
        assert int(s["is_static"]) == 0 and int(s["n_active"]) == d["n_active"], where
        assert int(s["mc"]) == int(d["mc"]), where
        assert int(s["n_rounds"]) == len(d["rounds"]), where
        for rd in d["rounds"]:
            j = rd["index"]
            got = (int(s["form"][j]), int(r["n_cols"][j]), int(r["n_rows"][j]), int(r["any_special"][j]))
            want = (FORM_CODE[rd["form"]], rd["n_cols"], rd["n_rows"], int(rd["any_special"]))
            assert got == want, "%s round %d: (form, n_cols, n_rows, any_special) is %s, declared %s" % (where, j, got, want)


def check_picture(name, i, pic):
    w, h, mbs, co = pic["w"], pic["h"], pic["mbs"], pic["coeffs"]
    is_p = bool(pic["base"])
    ref = fc.flat_reference()[2] if is_p else None
    want = expected(name, i, pic)
    check_fixture_blocks(pic, want, "the C oracle")
    # the declaration against the restatement from the LEVELs (wave_cases.anatomy)
    for a, d in zip(wc.anatomy(pic), pic["decl"]):
        assert (a["n_active"], a["forms"], a["mc"]) == (d["n_active"], [rd["form"] for rd in d["rounds"]], d["mc"]), (pic["table"], pic["tag"], a["mby"])
    for events in (False, True):
        for sparse in ((False, True) if is_p else (False,)):
            what = "%s coefficients, %s records" % ("events" if events else "dense", "sparse" if sparse else "dense")
            status, got = simlib.recon(w, h, mbs, co, ref, events=events, sparse_records=sparse)
            assert status == 0, what
            diff = wc.first_difference(pic, got, want)
            assert diff is None, "kernel phases on the CPU, %s: %s" % (what, diff)
            check_stats(pic, what)


@pytest.mark.parametrize("name", fc.TABLES)
def test_table(name):
    cov = fc.Coverage()
    pics = fc.table(name)
    assert pics
    for i, pic in enumerate(pics):
        check_picture(name, i, pic)
        cov.add(pic)
    assert cov.missing((name,)) == []


def test_coverage_reports_nothing_missing():
    cov = fc.Coverage()
    for _, _, pic in fc.all_pictures():
        cov.add(pic)
    assert cov.missing() == []


def test_the_coverage_notices_a_missing_case():
    """the zero-missing conditions are not vacuous: a kind dropped from a table is reported"""
    cov = fc.Coverage()
    for pic in fc.table_a(tuple(k for k in fc.KINDS if k != "horiz")):
        cov.add(pic)
    assert ("a", "horiz", "fma", "slot", 0) in cov.missing(("a",))
    cov = fc.Coverage()
    for pic in fc.table_e(tuple(k for k in fc.FULL_KINDS if k != "dense")):
        cov.add(pic)
    assert any(m[:2] == ("e", "dense") for m in cov.missing(("e",)))


def test_every_form_holds_blocks_listed_for_every_mutation():
    """what tests/test_gpu_mutation.py relies on: general-first, general-later, dense and wide rounds each hold fixture blocks
    the model lists for `pairwise` and for `fma`"""
    forms = {}
    for _, _, pic in fc.all_pictures():
        for _, _, _, e, mby, r, _ in pic["placed"]:
            for mu in e["detects"]:
                forms.setdefault((fc.form_name(pic["decl"][mby]["rounds"][r]), mu), set()).add(e["id"])
    for form in fc.FORM_NAMES:
        for mu in fc.MUTATIONS:
            assert len(forms.get((form, mu), ())) >= 8, (form, mu)


def detections(decoded, mutation):
    """decoded: [(picture, the oracle's planes, some build's planes)] -> {form name: [listed, differing from the oracle, equal to
    the model's prediction]} over the fixture blocks the model lists for that mutation (shared with tests/test_gpu_mutation.py)"""
    out = {form: [0, 0, 0] for form in fc.FORM_NAMES}
    for pic, want, got in decoded:
        w_views, g_views = wc.plane_views(pic, want), wc.plane_views(pic, got)
        for k, x, y, e, mby, r, slot in pic["placed"]:
            if mutation not in e["detects"]:
                continue
            n = out[fc.form_name(pic["decl"][mby]["rounds"][r])]
            blk = g_views[k][y:y + 8, x:x + 8]
            n[0] += 1
            n[1] += bool((blk != w_views[k][y:y + 8, x:x + 8]).any())
            n[2] += bool((blk == fc.expected_block(e, pic["base"], mutation)).all())
    return out


def test_the_pairwise_model_predicts_the_mutant_checker_build_in_every_form():
    """the checker built with -DH263MI_MUTATE_PAIRWISE: in the first general round, the later general rounds, dense rounds and
    wide rounds alike, the blocks the model lists differ from the oracle, and they are what the model says (the `n <= 1` exit
    lies behind the mutant's branch and the scalings by powers of two are exact, so one model serves every form)"""
    decoded = []
    for name, i, pic in fc.all_pictures():
        status, got = simlib.recon(pic["w"], pic["h"], pic["mbs"], pic["coeffs"], fc.flat_reference()[2] if pic["base"] else None,
                                   variant="pairwise")
        assert status == 0
        decoded.append((pic, expected(name, i, pic), got))
    for form, (listed, differ, agree) in detections(decoded, "pairwise").items():
        print("pairwise, %s: %d listed placements, %d differ from the oracle, %d equal the model" % (form, listed, differ, agree))
        assert listed >= 8 and differ == listed and agree == listed, (form, listed, differ, agree)


# ---------------------------------------------------------------------------------------------------------------
# the fixture
# ---------------------------------------------------------------------------------------------------------------
def test_the_forms_fixture_is_consistent():
    """every entry is of its kind, the C oracle and the soft-float model give `residual`, the mutated model gives the listed
    pixels, and every non-exempt (kind, mutation) has at least eight blocks: one per slot of a round"""
    from test_softfloat_oracle import c_block, clip255
    import sys
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(fc.HERE), "tools"))
    import find_sensitive_blocks as finder
    fx = fc.fixtures()
    assert fc.exempt() == {("corner2", "pairwise")}
    count = {}
    for kind in fc.NEW_KINDS:
        intra = kind in fc.INTRA_KINDS
        lo, hi = (1, 254) if intra else (-128, 127)
        for e in fx[kind]:
            assert kind in finder.kind_of(e["levels"], intra), e["id"]
            co = [sf.dequant(l, e["quant"]) if l else 0 for l in e["levels"]]
            if intra:
                assert e["levels"][0] == 0 and e["intradc"] not in (0, 128, 255)
                co[0] = 8 * e["intradc"]
            assert sf.classify(co)[0] == {"vert": "vert", "horiz": "horiz"}.get(kind, "full")
            assert (c_block(co) == clip255(e["residual"])).all(), e["id"]
            assert sf.block_residual(co) == e["residual"], e["id"]
            assert e["detects"]
            for mode, pixels in e["detects"].items():
                assert (kind, mode) not in fc.exempt() and pixels
                mut = sf.block_residual(co, mode)
                for y, x, v in pixels:
                    assert mut[y][x] == v != e["residual"][y][x]
                    assert lo <= v <= hi and lo <= e["residual"][y][x] <= hi
                count[(kind, mode)] = count.get((kind, mode), 0) + 1
    for kind, mu in fc.pairs():
        if kind != "full":
            assert count.get((kind, mu), 0) >= 8, (kind, mu, count.get((kind, mu), 0))


def test_the_exempt_pair_cannot_be_changed_by_its_mutation():
    """corner2 / pairwise: with two terms per sum the balanced tree is the sequential sum -- on 200 random corner2 blocks the
    pairwise model equals the reference model on every pixel"""
    import sys
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(fc.HERE), "tools"))
    import find_sensitive_blocks as finder
    levels, quant, code = finder.make_kind_blocks(np.random.default_rng(77), "corner2", 2000)
    co = finder.coefficients(levels, quant, code)
    for b in range(0, 2000, 10):
        c = [int(v) for v in co[b]]
        assert sf.block_residual(c, "pairwise") == sf.block_residual(c)
