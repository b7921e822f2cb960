"""The deblocking post-filter swept over every quartet class, tile kind and path -- on the CPU.

Three implementations must agree on every byte of the designed tables of tests/post_cases.py: the C oracle
(oracle/h263_oracle.c), the independent numpy restatement (oracle/np_restatement.py: deblock_trace, written from
deblock.rs) and the kernel phases themselves, compiled for the CPU (tests/sim/sim.cpp: sim_post, interior and general
instantiations).  The coverage conditions of both tables are asserted HERE, without a GPU: a table that stopped reaching a
class or a tile kind fails like a wrong byte does.  The three post-filter mutants of csrc/mutants.h, built into the
checker, must each differ from the oracle and equal its numpy model on every byte (the same assertion
tests/test_gpu_mutation.py makes of the gfx950 builds).

(Not here: a run under the AddressSanitizer build of the checker, and the layout / YUV shapes, for which the checker has
no entry; tests/test_sim_kernels.py keeps its sanitizer runs of sim_post.)"""
import json
import os

import numpy as np
import pytest

import post_cases as pc
import post_mutation_probe as probe
import simlib
from oracle import np_restatement as npr
from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
STRENGTHS = list(range(1, 13))


# ---------------------------------------------------------------------------------------------------------------
# the second opinion itself
# ---------------------------------------------------------------------------------------------------------------
SIZES = [(11, 17), (16, 16), (100, 60), (9, 9), (10, 10), (8, 2), (1, 1), (200, 37), (136, 40), (960, 20)]   # test_post_deblock_planes


@pytest.mark.parametrize("w,h", SIZES)
def test_restatement_equals_the_oracle_at_every_strength(w, h):
    rng = np.random.default_rng(w * 1000 + h)
    planes = [rng.integers(0, 256, w * h, dtype=np.uint8), np.clip(rng.normal(128, 7, w * h), 0, 255).astype(np.uint8),
              np.clip(rng.normal(250, 9, w * h), 0, 255).astype(np.uint8), np.clip(rng.normal(4, 9, w * h), 0, 255).astype(np.uint8)]
    for s in STRENGTHS:
        for p in planes:
            got, after_h, trace = npr.deblock_trace(p, w, s)
            diff = pc.first_difference("%dx%d" % (w, h), "numpy restatement (got) against the C oracle", w, h, got, orc.deblock(p, w, s), p, s)
            assert diff is None, diff
            # the trace is the filter: applying its quartets, pass by pass, to the input gives the same planes
            q = p.reshape(h, w).copy()
            for direction in (pc.DIR_H, pc.DIR_V):
                t = trace[trace["dir"] == direction]
                if direction == pc.DIR_V:
                    assert (q.ravel() == after_h).all()
                for k, o in enumerate(npr.process_quartets(*(t["abcd"][:, i] for i in range(4)), s, t["floor"])):
                    q[t["y"] + (k if direction == pc.DIR_H else 0), t["x"] + (0 if direction == pc.DIR_H else k)] = o
            assert (q.ravel() == got).all()


def test_restatement_on_the_reference_s_own_vectors():
    g = json.load(open(os.path.join(GOLD, "deblock_reference_tests.json")))
    img = g["image"]
    data = np.array(img["data"], np.uint8)
    for s in ("4", "8", "12"):
        assert npr.deblock(data, img["width"], int(s)).tolist() == img["expected"][s]
    for r in g["process_rows"]:        # deblock.rs:352-439: process() is the scalar (truncating) form
        out = npr.process_quartets(*[np.array([v]) for v in r["in"]], r["strength"], False)
        assert [int(o[0]) for o in out] == r["out"], r
        # a row 16 wide and 1 high is one vertical-edge quartet in a truncation row
        row = np.full(16, r["in"][0], np.uint8)
        row[6:10] = r["in"]
        row[10:] = r["in"][3]
        assert npr.deblock(row, 16, r["strength"])[6:10].tolist() == r["out"], r


def test_trace_positions_and_division():
    """11 x 17 (deblock.rs:441-449): one horizontal edge (rows 6..9; columns 0..7 shift, 8..10 divide), one vertical edge
    (columns 6..9; rows 0..15 shift, row 16 divides); the second horizontal edge would need row 17"""
    data = np.array(json.load(open(os.path.join(GOLD, "deblock_reference_tests.json")))["image"]["data"], np.uint8)
    _, _, t = npr.deblock_trace(data, 11, 4)
    th, tv = t[t["dir"] == pc.DIR_H], t[t["dir"] == pc.DIR_V]
    assert len(th) == 11 and (th["y"] == 6).all() and th["x"].tolist() == list(range(11))
    assert th["floor"].tolist() == [True] * 8 + [False] * 3
    assert len(tv) == 17 and (tv["x"] == 6).all() and tv["y"].tolist() == list(range(17))
    assert tv["floor"].tolist() == [True] * 16 + [False]
    assert th["abcd"][0].tolist() == [0, 0, 20, 20] and tv["abcd"][7].tolist() == [1, 1, 10, 10]     # row 7 after the first pass


# ---------------------------------------------------------------------------------------------------------------
# table (a): arithmetic
# ---------------------------------------------------------------------------------------------------------------
def test_lattice_is_the_checker_s():
    L = pc.lattice()
    assert len(L) == (511 * 2) ** 2
    x, y = L[:, 0].astype(int) - L[:, 3], L[:, 2].astype(int) - L[:, 1]
    assert len(np.unique(x * 1000 + y)) == 511 * 511
    assert len(pc.lattice_keys()) == 1020 ** 2      # a difference of +-255 has one place only: its two ends are one quartet


CONFIG_IDS = ["%s-%s" % ("hv"[d], "floor" if f else "trunc") for d, f in pc.A_CONFIGS]


@pytest.mark.parametrize("config", range(len(pc.A_CONFIGS)), ids=CONFIG_IDS)
@pytest.mark.parametrize("strength", STRENGTHS)
def test_table_a_every_lattice_point_in_every_semantics_direction_and_half(strength, config):
    direction, floor = pc.A_CONFIGS[config]
    cov = pc.CoverageA(strength)
    for pic in pc.table_a(direction, floor):
        want = orc.deblock(pic["plane"], pic["w"], strength)
        got, _, trace = npr.deblock_trace(pic["plane"], pic["w"], strength)
        assert (trace["dir"] == direction).all() and (trace["floor"] == floor).all()
        diff = pc.first_difference(pic["name"], "numpy restatement (got) against the C oracle", pic["w"], pic["h"], got, want,
                                   pic["plane"], strength)
        assert diff is None, diff
        cov.add(trace)
        _, sim = simlib.post(pic["w"], pic["h"], (pic["plane"].ravel(), None, None), strength, want_rgba=False, luma_only=True)
        diff = pc.first_difference(pic["name"], "kernel phases on the CPU", pic["w"], pic["h"], sim[0], want, pic["plane"], strength)
        assert diff is None, diff
    assert cov.missing([(direction, floor)]) == []
    print("strength %d, %s: %d classes; quartets per (floor, direction, half): %s" % (
        strength, CONFIG_IDS[config], len(pc.class_space(strength, floor)), {k: sum(v.values()) for k, v in sorted(cov.classes.items())}))


def test_table_a_without_one_plane_fails_its_coverage():
    """the zero-missing condition is not vacuous: every plane of table (a) is necessary (each holds lattice points no other
    plane of its configuration holds in that half).  Removed here: a-h-trunc-07."""
    cov = pc.CoverageA(5)
    for pic in pc.table_a(pc.DIR_H, False):
        if pic["name"] != "a-h-trunc-07":
            cov.add(npr.deblock_trace(pic["plane"], pic["w"], 5)[2])
    missing = cov.missing([(pc.DIR_H, False)])
    assert missing and all(m[:2] == (False, pc.DIR_H) for m in missing)


# ---------------------------------------------------------------------------------------------------------------
# table (b): placement
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table_b():
    """[(picture, [per stream: (decoded planes, filtered planes, RGBA)])], all the oracle's"""
    out = []
    for pic in pc.table_b():
        w, h = pic["w"], pic["h"]
        cw = (w + 1) // 2
        per = []
        for (mbs, co), s in zip(pic["streams"], pic["strengths"]):
            rc, planes = orc.decode_picture(w, h, mbs, co, None)
            assert rc == 0
            filt = planes if s == 0 else tuple(orc.deblock(p, pw, s) for p, pw in zip(planes, (w, cw, cw)))
            per.append((planes, filt, orc.yuv420_to_rgba(*filt, w)))
        out.append((pic, per))
    return out


def coverage_b(table, without=()):
    cov = pc.CoverageB()
    for pic, per in table:
        if pic["name"] in without:
            continue
        for (planes, filt, rgba), s in zip(per, pic["strengths"]):
            cov.add_picture(pic["w"], pic["h"], planes, s, rgba)
    return cov


def test_table_b_every_tile_kind_plane_direction_and_half_sees_every_condition(table_b):
    cov = coverage_b(table_b)
    print(cov.report())
    assert cov.missing() == []
    assert cov.excluded == 0
    assert set(s for pic, _ in table_b for s in pic["strengths"]) == set(range(13))


def test_table_b_without_one_size_fails_its_coverage(table_b):
    """392 x 97 is the one size whose chroma 8-limit ends the interior before the luma one does (tile column 3: luma columns
    260..387 lie left of 392, chroma columns 130..193 do not lie left of 192): without it the classifier names that kind --
    a coverage assertion, not a pixel comparison, is what notices"""
    missing = coverage_b(table_b, without=("b-392x97",)).missing()
    assert missing and all(m[1] == "chroma_limit" for m in missing)
    # ... and the truncation columns live in the two sizes 390 wide alone
    missing = coverage_b(table_b, without=("b-390x100", "b-390x97")).missing()
    assert any(m[1] == "trunc_cols" for m in missing)


def test_table_b_restatement_equals_the_oracle(table_b):
    for pic, per in table_b:
        w, h = pic["w"], pic["h"]
        cw = (w + 1) // 2
        for k, ((planes, filt, rgba), s) in enumerate(zip(per, pic["strengths"])):
            if s:
                got = tuple(npr.deblock(p, pw, s) for p, pw in zip(planes, (w, cw, cw)))
                diff = pc.first_difference("%s stream %d" % (pic["name"], k), "numpy restatement (got) against the C oracle", w, h, got, filt, planes, s)
                assert diff is None, diff


@pytest.mark.parametrize("size", range(len(pc.SIZES_B)), ids=["%dx%d" % s for s in pc.SIZES_B])
def test_table_b_kernel_phases_on_the_cpu(table_b, size):
    """RGBA only (interior tiles take the instantiations without bounds handling) and RGBA + planes (the general form)"""
    pic, per = table_b[size]
    w, h = pic["w"], pic["h"]
    for k, ((planes, filt, rgba), s) in enumerate(zip(per, pic["strengths"])):
        name = "%s stream %d strength %d" % (pic["name"], k, s)
        got, _ = simlib.post(w, h, planes, s, want_planes=False)
        bad = np.flatnonzero(got != rgba)
        assert bad.size == 0, "%s, RGBA only: %d bytes differ, first pixel (x %d, y %d)" % (name, bad.size, bad[0] // 4 % w, bad[0] // 4 // w)
        got, got_planes = simlib.post(w, h, planes, s)
        diff = pc.first_difference(name, "kernel phases on the CPU, RGBA + planes", w, h, got_planes, filt, planes, s)
        assert diff is None, diff
        assert (got == rgba).all(), name


# ---------------------------------------------------------------------------------------------------------------
# the three mutants, built into the checker
# ---------------------------------------------------------------------------------------------------------------
def sim_run(variant):
    def deblock(plane, width, strength):
        p = np.ascontiguousarray(plane, np.uint8).ravel()
        return simlib.post(width, p.size // width, (p, None, None), strength, want_rgba=False, luma_only=True, variant=variant)[1][0]

    def render(w, h, mbs, co, strength):
        rc, planes = orc.decode_picture(w, h, mbs, co, None)
        assert rc == 0
        return simlib.post(w, h, planes, strength, want_rgba=False, variant=variant)[1]

    return probe.run_all(deblock, render)


@pytest.fixture(scope="module")
def probe_oracle():
    return probe.expectations()


def test_probe_pictures_through_the_product_checker_are_clean(probe_oracle):
    names, n = probe.compare(sim_run(None), probe_oracle)
    assert n == 0, names[:5]


@pytest.mark.parametrize("mutant", probe.MUTANTS)
def test_mutation_models_predict_the_mutant_checker_builds(mutant, probe_oracle):
    got = sim_run(mutant)
    model = probe.expectations(mutant)
    names, n = probe.compare(got, model)
    assert n == 0, "the %s mutant (got) against its model (expected): %d bytes differ, in %s" % (mutant, n, names[:5])
    names, n = probe.compare(got, probe_oracle)
    print("%s mutant: %d bytes differ from the oracle, in %d of %d planes; all as its model predicts" % (mutant, n, len(names), len(got)))
    assert n > 0, "the %s mutant went unnoticed" % mutant
    check_where_the_mutant_differs(mutant, got, probe_oracle)


def check_where_the_mutant_differs(mutant, got, oracle):
    """On the table (a) planes no quartet reads what another wrote, so the classifier says where a mutant may differ:
      dbhalf   exactly at the rounding-sensitive quartets, A and D by one (mod 256), B and C untouched
      dbfloor  only in truncation planes, and only at quartets whose numerators are division-sensitive or whose d1 is
               negative and odd (its half rounds the other way too)
      dbwrap   only in columns 0..3 of the one plane whose columns ride (8 wide), rows of horizontal edges"""
    for pic in probe.planes_a():
        w, h = pic["w"], pic["h"]
        g, e = got[pic["name"]].reshape(h, w), oracle[pic["name"]].reshape(h, w)
        trace = npr.deblock_trace(pic["plane"], w, probe.PROBE_STRENGTH)[2]
        cls = pc.classify(trace["abcd"], trace["floor"], probe.PROBE_STRENGTH)
        is_h = trace["dir"] == pc.DIR_H
        delta = np.stack([(g[trace["y"] + np.where(is_h, k, 0), trace["x"] + np.where(is_h, 0, k)].astype(int) -
                           e[trace["y"] + np.where(is_h, k, 0), trace["x"] + np.where(is_h, 0, k)]) for k in range(4)], axis=1)
        differs = delta.any(axis=1)
        assert int((g != e).sum()) == int((delta != 0).sum())          # nothing differs outside the quartets
        if mutant == "dbhalf":
            assert (differs == cls["roundsens"]).all(), pic["name"]
            d = delta[differs]
            da, dd = (d[:, 0] + 128) % 256 - 128, (d[:, 3] + 128) % 256 - 128      # (A and D wrap: deblock.rs:38,41)
            assert (len(d) > 0) == pic["floor"] and (np.abs(da) == 1).all() and (dd == -da).all() and not d[:, 1:3].any(), pic["name"]
        elif mutant == "dbfloor":
            if pic["floor"]:
                assert not differs.any(), pic["name"]
            else:
                S = probe.PROBE_STRENGTH
                m = np.abs(npr._div_pow2(trace["abcd"].astype(int) @ np.array([1, -4, 4, -1]), 3, False))
                odd_neg = (cls["sign"] < 0) & (np.maximum(m - np.maximum(2 * (m - S), 0), 0) % 2 == 1)
                assert differs.any() and (differs <= ((cls["divsens"] != 0) | odd_neg)).all(), pic["name"]
        else:
            wrapped = pc.post_tile_columns(w)[1] == 1
            if not wrapped:
                assert not differs.any(), pic["name"]
            else:
                assert differs.any() and (trace["x"][differs] < 4).all() and is_h[differs].all()
                # every quartet of those columns that the reference changes at all is left as it was
                changed = (e != pic["plane"])[:, :4].any()
                assert changed and (g[:, :4] == pic["plane"][:, :4]).all() and (g[:, 4:] == e[:, 4:]).all()


def test_the_product_build_defines_none_of_the_switches():
    """each mutant is one -D of its own on the mutants' rule; the product's flags name none (csrc/mutants.h: every switch is
    then a compile-time false)"""
    root = os.path.dirname(HERE)
    mk = open(os.path.join(root, "h263-rs_amd", "Makefile")).read()
    hdr = open(os.path.join(root, "h263-rs_amd", "csrc", "mutants.h")).read()
    flags = [ln for ln in mk.splitlines() if ln.startswith("HIPFLAGS")]
    assert len(flags) == 1 and "MUTATE" not in flags[0]
    for name, macro in (("dbhalf", "H263MI_MUTATE_DEBLOCK_HALF_ROUNDING"), ("dbfloor", "H263MI_MUTATE_DEBLOCK_FLOOR_EVERYWHERE"),
                        ("dbwrap", "H263MI_MUTATE_DEBLOCK_WRAP_COLUMNS")):
        assert [ln for ln in mk.splitlines() if ln.startswith("MUTFLAGS_" + name)][0].split("=", 1)[1].strip() == "$(HIPFLAGS) -D" + macro
        assert name in [ln for ln in mk.splitlines() if ln.startswith("MUTANTS =")][0].split()
        assert "defined(%s)" % macro in hdr
        assert macro in open(os.path.join(simlib.SIM_DIR, "Makefile")).read()
