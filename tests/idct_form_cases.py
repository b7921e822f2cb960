"""Designed cases for the ARITHMETIC of a reconstruction round: blocks on which a fused or re-associated IDCT changes a pixel
(the two mutation fixtures under tests/golden/, found with the FPU-free soft-float model) placed so that they pass through
every form the round's code is compiled in -- the counterpart of tests/wave_cases.py, which does the same for the bookkeeping.

INPUTS ONLY, plus a DECLARATION: this file builds macroblock records and coefficient pools, and says for every round of every
wave which form it must take (general / dense / wide), the extent of its truncated sums (n_cols, n_rows), whether its column
pass applies the class fix-up (any_special), whether the wave takes a prediction (MC) or is all-intra, the round's index and
which slot holds which fixture block.  The declaration is made from the KINDS of the blocks placed (what each kind is by
construction: DESIGN.md section 3 and rle.rs:138-171), never from a kernel or from the CPU checker: the tests hold the
checker's own report against it.  Expected pixels never come from here: they are the C oracle's, and inside a fixture block
additionally clamp(base + the fixture's soft-float residual).

Pictures are one wave wide and four macroblock rows high (128 x 64), every macroblock row one wave.  P pictures are decoded
over a flat key frame of 128 (every INTRADC code 255), all vectors zero; I pictures have nothing underneath (base 0).

A wave is given as a grid[macroblock 0..7][block 0..5] of block specifications (None: not coded).  Task order and ranks are
those of wave_cases: luma block row 0 (blocks 0, 1 of macroblocks 0..7), luma block row 1 (blocks 2, 3), Cb, Cr; the active
blocks in that order fill rounds of eight.  With only blocks out of {0, 2, 4, 5} in use, the j-th of them is round j and the
macroblock is the slot.  The six blocks of a macroblock share its quantiser; the new fixture uses few quantisers for that.

A block specification is ("fx", entry) for a fixture block or one of the companions:
  "dc"       an inter block with one LEVEL at position 0                                  (the Dc class)
  "vert"     an inter block with LEVELs at positions 0 and 16                             (the Vert class, three rows)
  "zero"     a coded block whose LEVELs are all zero: the Zero class INSIDE a round.  (A killed block is Zero for the
             reference, rle.rs:125-127; the mark phase drops it, so it holds a pool slot and no slot of a round.)
  "killed"   that: coded and killed, idle
  "full77"   a Full block with a LEVEL at (7, 7): widens every sum of its round to eight terms
  "breaker"  a Full block with one LEVEL at (1, 1): it breaks the dense condition
  "wide+" / "wide-"   a Full block with the LEVEL 600 / -700 at (2, 2), as wave_cases.wide_block: its round is wide
  "idc"      an uncoded block of an intra macroblock with a legal INTRADC: the Dc class from INTRADC, no pool slot

The tables:
  (a) waves of 48 blocks of one kind: every slot and every round index
  (b) the corner kinds alone (extent c x c) and beside "full77" (8 x 8)
  (c) Full kinds beside Dc, Vert, Zero and all three; vert and horiz kinds beside Full companions
  (d) seven dense blocks and a breaker (general), followed by a dense round; the same all-intra   [dense rounds proper: (a)]
  (e) every Full kind beside a wide companion in slot 0 and in slot 7
  (f) intra_full alone and beside "idc" blocks
  (g) single blocks alone in their waves: every extent the kinds without a fixed one hold
"""
import json
import os

import numpy as np

import wave_cases as wc

HERE = os.path.dirname(os.path.abspath(__file__))
GENERAL, DENSE, WIDE = wc.GENERAL, wc.DENSE, wc.WIDE
W, ROWS = 128, 4
H = 16 * ROWS
MUTATIONS = ("fma", "pairwise")
NEW_KINDS = ("corner2", "corner4", "corner6", "vert", "horiz", "dense", "intra_full", "intra_dense")
KINDS = ("full",) + NEW_KINDS                                    # "full": the blocks of idct_sensitive_blocks.json
INTRA_KINDS = ("intra_full", "intra_dense")
FULL_KINDS = ("full", "corner2", "corner4", "corner6", "dense", "intra_full", "intra_dense")
CORNER = {"corner2": 2, "corner4": 4, "corner6": 6}
TABLES = ("a", "b", "c", "d", "e", "f", "g")
WIDE_MAX_QUANT = 8                                               # 8 * (2 * 700 + 1) = 11208: the reference's i16 product holds


# ---------------------------------------------------------------------------------------------------------------
# the fixtures
# ---------------------------------------------------------------------------------------------------------------
_FX = {}


def fixtures():
    """{kind: [entry]}; every entry knows its kind and its index within the kind ("id")"""
    if not _FX:
        old = json.load(open(os.path.join(HERE, "golden", "idct_sensitive_blocks.json")))["blocks"]
        new = json.load(open(os.path.join(HERE, "golden", "idct_sensitive_forms.json")))
        for e in old:
            e["kind"] = "full"
        by_kind = {}
        for e in old + new["blocks"]:
            by_kind.setdefault(e["kind"], []).append(e)
        for kind, es in by_kind.items():
            # the blocks listed for one mutation and for the other by turns, so that any few of them in a row hold both
            lists = [[e for e in es if mu in e["detects"] and (mu == "fma" or "fma" not in e["detects"])] for mu in MUTATIONS]
            es = [l[i] for i in range(max(map(len, lists))) for l in lists if i < len(l)]
            for i, e in enumerate(es):
                e["id"] = (kind, i)
            _FX[kind] = es
        _FX["exempt"] = {tuple(p) for p in new["exempt"]}
    return _FX


def exempt():
    return fixtures()["exempt"]


def pairs():
    """the (kind, mutation) pairs that must be covered"""
    return [(k, mu) for k in KINDS for mu in MUTATIONS if (k, mu) not in exempt()]


def by_quant(kind, most=31):
    out = {}
    for e in fixtures()[kind]:
        if e["quant"] <= most:
            out.setdefault(e["quant"], []).append(e)
    return out


def take(kind, n, start=0, most=31):
    """n fixture blocks of a kind, one after the other from `start` (around the end)"""
    es = [e for e in fixtures()[kind] if e["quant"] <= most]
    return [es[(start + i) % len(es)] for i in range(n)]


# ---------------------------------------------------------------------------------------------------------------
# what a block specification IS (by its kind) and its LEVELs
# ---------------------------------------------------------------------------------------------------------------
def fx(entry):
    return ("fx", entry)


def spec_levels(spec, intra):
    c = np.zeros(64, np.int16)
    what = spec[0] if isinstance(spec, tuple) else spec
    if what == "fx":
        c[:] = spec[1]["levels"]
    elif what == "dc":
        c[0] = 2
    elif what == "vert":
        c[0], c[16] = 1, -2
    elif what == "full77":
        c[63] = 1
    elif what == "breaker":
        c[9] = 2
    elif what in ("wide+", "wide-"):
        c[18] = 600 if what == "wide+" else -700
    elif what not in ("zero", "killed"):
        raise ValueError(what)
    if intra:
        assert c[0] == 0 or what != "fx"
        c[0] = 0
    return c


def own_extent(levels, intra):
    """(n_cols, n_rows) a block asks of its round: the coefficient columns count in pairs and are at least two, the rows are at
    least one; an intra block's DC (INTRADC, never 0 here) stands in row 0"""
    g = np.asarray(levels).reshape(8, 8) != 0
    rows = [r for r in range(8) if g[r].any()]
    pairs_ = [j for j in range(4) if g[:, 2 * j:2 * j + 2].any()]
    return 2 * (1 + max(pairs_ + [0])), 1 + max(rows + [0])


def spec_facts(spec, intra):
    """(class, (n_cols, n_rows), may be part of a dense round, makes its round wide) -- by the KIND of the specification"""
    what = spec[0] if isinstance(spec, tuple) else spec
    if what == "fx":
        kind = spec[1]["kind"]
        assert (kind in INTRA_KINDS) == intra
        if kind in CORNER:
            return "full", (CORNER[kind], CORNER[kind]), False, False
        if kind in ("dense", "intra_dense"):
            return "full", (8, 8), True, False
        return (kind if kind in ("vert", "horiz") else "full"), own_extent(spec[1]["levels"], intra), False, False
    return {"dc": ("dc", (2, 1), False, False), "idc": ("dc", (2, 1), False, False), "zero": ("zero", (2, 1), False, False),
            "vert": ("vert", (2, 3), False, False), "full77": ("full", (8, 8), False, False),
            "breaker": ("full", (2, 2), False, False), "wide+": ("full", (4, 3), False, True),
            "wide-": ("full", (4, 3), False, True)}[what]


# ---------------------------------------------------------------------------------------------------------------
# building a picture and its declaration
# ---------------------------------------------------------------------------------------------------------------
def empty_grid():
    return [[None] * 6 for _ in range(wc.WAVE_MBS)]


def column_grid(rounds, blocks=(0, 2, 4, 5)):
    """rounds: up to four lists of eight specifications -> a grid in which list j is round j and the macroblock is the slot"""
    g = empty_grid()
    for j, specs in enumerate(rounds):
        assert len(specs) == 8
        for m, s in enumerate(specs):
            g[m][blocks[j]] = s
    return g


def build(table, grids, intra, **tag):
    """one picture of ROWS waves (missing ones: nothing coded).  Returns the picture: table / w / h / mbs / coeffs /
    picture_type / tag / loud as wave_cases' pictures, plus
      decl     per macroblock row {"mc", "n_active", "rounds": [{"index", "form", "n_cols", "n_rows", "any_special",
               "slots": [specification or None] * 8, "classes": {...}}]}
      placed   [(plane, x, y, entry, macroblock row, round index, slot)] of the fixture blocks"""
    assert len(grids) <= ROWS
    grids = list(grids) + [empty_grid()] * (ROWS - len(grids))
    rows, pool, decl, placed = [], [], [], []
    for mby, g in enumerate(grids):
        specs_row, active = [], []
        for m in range(wc.WAVE_MBS):
            qs = {s[1]["quant"] for s in g[m] if isinstance(s, tuple)}
            assert len(qs) <= 1, "the blocks of a macroblock share its quantiser: %s" % sorted(qs)
            q = qs.pop() if qs else 1
            cbp = kill = 0
            dc = [0] * 6
            for b, s in enumerate(g[m]):
                if s is None:
                    continue
                what = s[0] if isinstance(s, tuple) else s
                if what == "idc":
                    assert intra
                    dc[b] = wc.legal_dc(17 * m + 5 * b + mby)
                    continue
                cbp |= 1 << b
                if what == "killed":
                    kill |= 1 << b
                if intra:
                    dc[b] = s[1]["intradc"] if what == "fx" else wc.legal_dc(11 * m + 3 * b + mby)
                lv = spec_levels(s, intra)
                assert (q * (2 * np.abs(lv.astype(np.int64)) + 1) <= 32767).all(), "the reference's i16 product must not overflow"
            specs_row.append(wc.mb(wc.INTRA if intra else wc.INTER, cbp, kill, 0, dc, q))
            for b in range(6):                                   # the pool: coded blocks in raster order, killed ones too
                if (cbp >> b) & 1:
                    pool.append(spec_levels(g[m][b], intra))
        for t in range(wc.WAVE_TASKS):                           # the active blocks in task order fill rounds of eight
            s = g[wc.task_mb(t)][wc.task_blk(t)]
            if s is not None and s != "killed":
                active.append((t, s))
        rounds = []
        for r in range((len(active) + 7) // 8):
            part = active[8 * r:8 * r + 8]
            facts = [spec_facts(s, intra) for _, s in part]
            wide = any(f[3] for f in facts)
            dense = not wide and len(part) == 8 and all(f[2] for f in facts)
            classes = {f[0] for f in facts}
            rounds.append({"index": r, "form": WIDE if wide else DENSE if dense else GENERAL,
                           "n_cols": 8 if dense else max(f[1][0] for f in facts),
                           "n_rows": 8 if dense else max(f[1][1] for f in facts),
                           "any_special": not dense and bool(classes - {"full"}),
                           "slots": [s for _, s in part] + [None] * (8 - len(part)), "classes": classes})
            for slot, (t, s) in enumerate(part):
                if isinstance(s, tuple):
                    placed.append(wc.task_region(t, mby, 0) + (s[1], mby, r, slot))
        decl.append({"mc": not intra, "n_active": len(active), "rounds": rounds})
        rows.append(specs_row)
    mbs, _ = wc.records_of(W, H, rows)
    co = np.array(pool, np.int16).reshape(-1, 64)
    return {"table": table, "w": W, "h": H, "mbs": mbs, "coeffs": co, "picture_type": wc.PICTURE_I if intra else wc.PICTURE_P,
            "tag": tag, "loud": set(range(len(co))), "decl": decl, "placed": placed, "base": 0 if intra else 128}


def pictures_of(table, grids, intra, **tag):
    """as many pictures as the waves need, ROWS waves each"""
    return [build(table, grids[at:at + ROWS], intra, part=at // ROWS, **tag) for at in range(0, len(grids), ROWS)]


def flat_reference(w=W, h=H):
    """(records, coefficients, planes) of the key frame of the P pictures: every pixel 128"""
    from oracle.oracle import MB_RECORD_DTYPE
    mbw, mbh = wc.mb_dims(w, h)
    mbs = np.zeros(mbw * mbh, MB_RECORD_DTYPE)
    mbs["mb_type"], mbs["quant"], mbs["intradc"] = wc.INTRA, 1, 255
    cw, ch = (w + 1) // 2, (h + 1) // 2
    return mbs, np.zeros((0, 64), np.int16), (np.full(w * h, 128, np.uint8), np.full(cw * ch, 128, np.uint8), np.full(cw * ch, 128, np.uint8))


def expected_block(entry, base, mutation=None):
    """clamp(base + residual) of a fixture block, [y][x]; with a mutation's name, what the model says that mutation makes"""
    res = np.array(entry["residual"], np.int32)
    if mutation and mutation in entry["detects"]:
        for y, x, v in entry["detects"][mutation]:
            res[y, x] = v
    return np.clip(base + res, 0, 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------------------------
A_WAVES = 4


def table_a(kinds=KINDS):
    """waves of 48 blocks of one kind: macroblock m of wave r takes one quantiser of the kind and six of its blocks, moving on
    with r, so that the blocks a mutation is listed for pass through every slot and every round index"""
    for kind in kinds:
        groups = by_quant(kind)
        quants = sorted(groups)
        grids, at = [], {q: 0 for q in quants}
        for r in range(A_WAVES):
            g = empty_grid()
            for m in range(wc.WAVE_MBS):
                q = quants[(3 * r + m) % len(quants)]
                for b in range(6):
                    g[m][(b + r) % 6] = fx(groups[q][at[q] % len(groups[q])])
                    at[q] += 1
            grids.append(g)
        yield from pictures_of("a", grids, kind in INTRA_KINDS, kind=kind)


def table_b(kinds=tuple(CORNER)):
    """two rounds of a corner kind alone (the extent is c x c), then the same with one "full77" in slot 3 / slot 6 (8 x 8)"""
    for kind in kinds:
        first = [fx(e) for e in take(kind, 8)]
        own = [first, _same_quant(first, kind, 1)]               # (the two rounds of a macroblock share its quantiser)
        wid = [list(first), _same_quant(first, kind, 2)]
        wid[0][3] = wid[1][6] = "full77"
        yield from pictures_of("b", [column_grid(own), column_grid(wid)], False, kind=kind)


def _same_quant(first, kind, step):
    """for every slot a block of the kind with the quantiser of the block `first` holds there (another one where there is one)"""
    groups = by_quant(kind)
    out = []
    for m, s in enumerate(first):
        if not isinstance(s, tuple):
            out.append(fx(take(kind, 1, m)[0]))
            continue
        grp = groups[s[1]["quant"]]
        out.append(fx(grp[(grp.index(s[1]) + step) % len(grp)]))
    return out


C_MIXES = (("dc",), ("vert",), ("zero",), ("dc", "vert", "zero"))
C_KINDS = ("full", "corner2", "corner4", "corner6", "dense")


def table_c():
    """Full kinds beside the special classes: one round per mix, the companions in the last slots (and a killed block among
    the first, which takes a pool slot and no slot of the round); vert and horiz kinds beside Full companions"""
    for kind in C_KINDS:
        grids = []
        for i, mix in enumerate(C_MIXES):
            specs = [fx(e) for e in take(kind, 8 - len(mix), 8 * i)] + list(mix)
            specs = specs[-i:] + specs[:-i] if i else specs         # (the companions' slots move)
            g = column_grid([specs])
            if "zero" in mix:
                g[1][1] = "killed"
            grids.append(g)
        yield from pictures_of("c", grids, False, kind=kind)
    for kind in ("vert", "horiz"):
        grids = []
        for i, companion in enumerate(("breaker", "full77")):
            specs = [fx(e) for e in take(kind, 8, 6 * i)]
            specs[(2 + 3 * i) % 8] = specs[(5 + 3 * i) % 8] = companion
            grids.append(column_grid([specs]))
        yield from pictures_of("c", grids, False, kind=kind)


def table_d():
    """seven dense blocks and one that breaks the condition: a general round; a dense round behind it"""
    for kind in ("dense", "intra_dense"):
        first = [fx(e) for e in take(kind, 8, 2)]
        first[5] = "breaker"
        second = _same_quant(first, kind, 1)
        yield from pictures_of("d", [column_grid([first]), column_grid([first, second])], kind in INTRA_KINDS, kind=kind)


def table_e(kinds=FULL_KINDS):
    """every Full kind beside one block with a LEVEL outside [-512, 511]: in slot 0 of round 0 and in slot 7 of round 1"""
    for kind in kinds:
        grids = []
        for i, companion in enumerate(("wide+", "wide-")):
            first = [fx(e) for e in take(kind, 8, 4 * i, WIDE_MAX_QUANT)]
            second = _same_quant(first, kind, 2)
            first[0], second[7] = companion, companion
            grids.append(column_grid([first, second]))
        yield from pictures_of("e", grids, kind in INTRA_KINDS, kind=kind)


def table_f():
    """all-intra general rounds: intra_full alone, and beside uncoded intra blocks (the Dc class from INTRADC)"""
    alone = [fx(e) for e in take("intra_full", 8, 1)]
    beside = [fx(e) for e in take("intra_full", 8, 9)]
    beside[1] = beside[6] = "idc"
    later = _same_quant(alone, "intra_full", 2)
    later[0] = later[3] = "idc"
    yield from pictures_of("f", [column_grid([alone]), column_grid([beside]), column_grid([alone, later])], True, kind="intra_full")


FORM_NAMES = ("general-first", "general-later", "dense", "wide")


def form_name(rd):
    """the four stretches of machine code the mutants are looked for in: the general form is compiled twice (the peeled first
    round and the loop of the later ones)"""
    if rd["form"] == GENERAL:
        return "general-first" if rd["index"] == 0 else "general-later"
    return rd["form"]


G_KINDS = ("full", "vert", "horiz", "intra_full")


def own_extents(kind):
    """{(n_cols, n_rows): the first fixture block of the kind that asks for it}"""
    out = {}
    for e in fixtures()[kind]:
        out.setdefault(own_extent(e["levels"], kind in INTRA_KINDS), e)
    return out


def table_g(kinds=G_KINDS):
    """a block alone in its wave -- a round of one block, the other seven slots idle: the sums are truncated to the block's own
    extent, whatever it is (the kinds that do not fix it: one wave per extent the fixture holds)"""
    for kind in kinds:
        grids = []
        for i, (_, e) in enumerate(sorted(own_extents(kind).items())):
            g = empty_grid()
            g[(3 * i) % 8][(0, 3, 4, 1, 5, 2)[i % 6]] = fx(e)
            grids.append(g)
        yield from pictures_of("g", grids, kind in INTRA_KINDS, kind=kind)


GENERATORS = {"a": table_a, "b": table_b, "c": table_c, "d": table_d, "e": table_e, "f": table_f, "g": table_g}


def table(name):
    return list(GENERATORS[name]())


def all_pictures():
    return [(name, i, pic) for name in TABLES for i, pic in enumerate(table(name))]


# ---------------------------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------------------------
class Coverage:
    """what a set of pictures puts the fixture blocks through, by the DECLARATION of their waves.  The conditions are
    enumerations, not measurements."""

    def __init__(self):
        self.seen = set()      # (table, kind, mutation, form, round index, slot, "mc" / "intra", "own" / "widened", companion classes)

    def add(self, pic):
        for _, _, _, e, mby, r, slot in pic["placed"]:
            d = pic["decl"][mby]
            rd = d["rounds"][r]
            _, own, _, _ = spec_facts(fx(e), pic["base"] == 0)
            extent = "own" if (rd["n_cols"], rd["n_rows"]) == own else "widened"
            companions = frozenset(spec_facts(s, pic["base"] == 0)[0] + ("" if isinstance(s, tuple) else "*")
                                   for s in rd["slots"] if s is not None and not isinstance(s, tuple))
            wide_slot = [k for k, s in enumerate(rd["slots"]) if s in ("wide+", "wide-")]
            for mu in e["detects"]:
                self.seen.add((pic["table"], e["kind"], mu, rd["form"], r, slot, "mc" if d["mc"] else "intra", extent, companions,
                               wide_slot[0] if wide_slot else None, d["n_active"], (rd["n_cols"], rd["n_rows"])))

    def _have(self, **want):
        names = ("table", "kind", "mu", "form", "round", "slot", "wave", "extent", "companions", "wide_slot", "n_active", "size")
        return [dict(zip(names, s)) for s in self.seen if all(dict(zip(names, s))[k] == v for k, v in want.items())]

    def missing(self, tables=TABLES):
        out = []
        for kind, mu in pairs():
            intra = kind in INTRA_KINDS
            wave = "intra" if intra else "mc"
            form = DENSE if kind in ("dense", "intra_dense") else GENERAL
            if "a" in tables:
                got = self._have(table="a", kind=kind, mu=mu, form=form, wave=wave, n_active=48)
                out += [("a", kind, mu, "slot", s) for s in range(8) if s not in {g["slot"] for g in got}]
                out += [("a", kind, mu, "round", r) for r in range(6) if r not in {g["round"] for g in got}]
            if "b" in tables and kind in CORNER:
                for extent in ("own", "widened"):
                    for r in (0, 1):
                        if not self._have(table="b", kind=kind, mu=mu, form=GENERAL, extent=extent, round=r):
                            out.append(("b", kind, mu, extent, r))
            if "c" in tables and kind in C_KINDS:
                for mix in C_MIXES:
                    if not self._have(table="c", kind=kind, mu=mu, form=GENERAL, companions=frozenset(m + "*" for m in mix)):
                        out.append(("c", kind, mu, mix))
            if "c" in tables and kind in ("vert", "horiz"):
                if not self._have(table="c", kind=kind, mu=mu, form=GENERAL, companions=frozenset(["full*"])):
                    out.append(("c", kind, mu, "beside Full companions"))
            if "d" in tables and kind in ("dense", "intra_dense"):
                if not self._have(table="d", kind=kind, mu=mu, form=GENERAL, wave=wave, companions=frozenset(["full*"])):
                    out.append(("d", kind, mu, "seven dense blocks and a breaker: general"))
                if not self._have(table="d", kind=kind, mu=mu, form=DENSE, wave=wave, round=1):
                    out.append(("d", kind, mu, "a dense round behind a general one"))
            if "a" in tables and kind in ("dense", "intra_dense"):
                for what, rs in (("dense first round", (0,)), ("dense later round", (1, 2, 3, 4, 5))):
                    if not any(self._have(table="a", kind=kind, mu=mu, form=DENSE, wave=wave, round=r) for r in rs):
                        out.append(("a", kind, mu, what))
            if "e" in tables and kind in FULL_KINDS:
                for r, slot in ((0, 0), (1, 7)):
                    if not self._have(table="e", kind=kind, mu=mu, form=WIDE, wave=wave, round=r, wide_slot=slot):
                        out.append(("e", kind, mu, "wide companion in slot %d of round %d" % (slot, r)))
            if "f" in tables and kind == "intra_full":
                if not self._have(table="f", kind=kind, mu=mu, form=GENERAL, wave="intra", companions=frozenset()):
                    out.append(("f", kind, mu, "alone"))
                if not self._have(table="f", kind=kind, mu=mu, form=GENERAL, wave="intra", companions=frozenset(["dc*"])):
                    out.append(("f", kind, mu, "beside uncoded intra blocks"))
        if "g" in tables:
            for kind in G_KINDS:
                out += [("g", kind, size) for size in sorted(own_extents(kind))
                        if not self._have(table="g", kind=kind, form=GENERAL, n_active=1, size=size, extent="own")]
        return out
