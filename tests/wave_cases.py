"""Designed cases for the BOOKKEEPING of a reconstruction wave, the anatomy of every wave, and the accounting of what the
cases exercise (records -> at most 48 block tasks -> compaction by ballot -> rounds of eight -> which
instantiation the wave takes).

INPUTS ONLY, plus a restatement of the DESIGN: this file builds macroblock records and coefficient pools (for
H263State.submit_picture, Batch.decode / decode_events / submit_host, simlib.recon and the oracles) and says, from the
records alone, what every wave of a picture is.  Expected pixels never come from here -- they are the C oracle's.  Nothing
is imported from the kernels or from the CPU checker: the anatomy is written from DESIGN.md section 3 and the reference's
semantics (rle.rs:125-127: a killed block is Zero; gather.rs:136-149: which macroblocks take a prediction; state.rs:207-216:
COD = 1 is Inter / vector 0 / nothing coded; state.rs:421-427: missing macroblocks likewise), and the tests hold the
checker's own report (sim_wave_stats) against it.

A wave is eight macroblocks of one macroblock row.  Block task t of a wave: t < 32 is a luma block -- block row t >> 4,
block column t & 15, i.e. macroblock (t >> 1) & 7, block ((t >> 4) << 1) | (t & 1) --, then the eight Cb blocks, then the
eight Cr blocks (macroblock t & 7, block 4 + ((t >> 3) & 1)).

The tables (generators of dicts: table / w / h / mbs / coeffs / picture_type / tag / loud):
  (a) table_a_p, table_a_i, table_a_dc   every mb_type x cbp x kill, shuffled; the intra ones again as I pictures; a strip of
                uncoded intra blocks with the INTRADC codes 0, 1, 127, 128, 129, 254, 255
  (b) table_b   every n_active 0..48 from the low and from the high end, every task alone, every task missing -- in
                all-intra waves of I pictures, all-inter waves and mixed waves --, and the round forms (dense, wide) placed
                among general rounds
  (c) table_c   widths of 1..17 and 24 macroblocks: static waves, near-static waves (one vector component +-1), waves with a
                single active block, the same in the right-edge wave of 1..7 macroblocks
  (d) table_d   (bitstream path) every mask of a full group beside every mask of a partial group of 1..7 macroblocks

Every coded block carries a SIGNATURE that depends on its index in the coefficient pool (one or two LEVELs of magnitude
<= 5 at positions cycling over 0 / 1 / 8 / 9; an intra block takes 2 for 0: its DC travels as INTRADC), so a block read
from a neighbouring pool slot changes pixels, and the magnitudes are held down at large quantisers so that no residual is
hidden by the final clamp over a mid-range reference (the CPU tests assert both).  `loud` names the pool blocks that are
not signatures (dense and wide blocks: their residuals may clamp).
"""
import numpy as np

from oracle.oracle import MB_RECORD_DTYPE

INTER, INTER_Q, INTER4V, INTRA, INTRA_Q, INTER4V_Q = range(6)
INTRA_TYPES, INTER_TYPES = (3, 4), (0, 1, 2, 5)
PICTURE_I, PICTURE_P = 0, 1
WAVE_MBS, WAVE_TASKS, ROUND_BLOCKS = 8, 48, 8
GENERAL, DENSE, WIDE = "general", "dense", "wide"
DC_EDGE_CODES = (0, 1, 127, 128, 129, 254, 255)
ALL_TASKS = (1 << WAVE_TASKS) - 1


def mb_dims(w, h):
    return (w + 15) // 16, (h + 15) // 16


def task_mb(t):
    return (t >> 1) & 7 if t < 32 else t & 7


def task_blk(t):
    return ((t >> 4) << 1) | (t & 1) if t < 32 else 4 + ((t >> 3) & 1)


TASK_OF = {(task_mb(t), task_blk(t)): t for t in range(WAVE_TASKS)}
assert len(TASK_OF) == WAVE_TASKS


def task_region(t, mby, group):
    """(plane, x, y) of the 8x8 pixels of task t of the wave at (macroblock row, group of 8)"""
    if t < 32:
        return 0, 128 * group + (t & 15) * 8, 16 * mby + (t >> 4) * 8
    return 1 + ((t >> 3) & 1), 64 * group + (t & 7) * 8, 8 * mby


def popcount(v):
    return bin(int(v)).count("1")


# ---------------------------------------------------------------------------------------------------------------
# building pictures
# ---------------------------------------------------------------------------------------------------------------
def legal_dc(i):
    """an INTRADC code of the middle of the range (never 0 or 128, which no bitstream carries)"""
    c = 64 + i % 128
    return 129 if c == 128 else c


def mb(t=INTER, cbp=0, kill=0, mv=0, dc=0, q=1, kinds=None):
    """one macroblock of a picture under construction; mv: one (x, y) for all four blocks or four of them; dc: one code or
    six; kinds: {block: DENSE / WIDE} for the coded blocks that are not signatures"""
    v = np.zeros((4, 2), np.int64)
    v[:] = np.asarray(mv).reshape(-1, 2) if np.ndim(mv) else mv
    d = np.zeros(6, np.int64)
    d[:] = dc
    return {"t": t, "cbp": cbp, "kill": kill, "mv": v, "dc": d, "q": q, "kinds": kinds or {}}


def _level(base, q):
    """the magnitude `base` (2..5), held down so that the dequantised value q (2 |L| + 1) stays within 130"""
    m = base
    while m > 1 and (2 * m + 1) * q > 130:
        m -= 1
    return m


def _position(j, intra):
    """positions cycle over 0 / 1 / 8 / 9; an intra block takes 2 where the cycle says 0 (its DC travels as INTRADC)"""
    p = (0, 1, 8, 9)[j % 4]
    return 2 if intra and p == 0 else p


def signature(k, intra, q):
    """the LEVELs of pool block k: one LEVEL, a second one for every third block.  Neighbours in the pool never share a
    position, whoever reads them"""
    c = np.zeros(64, np.int16)
    c[_position(k, intra)] = _level(2 + (k // 4) % 4, q) * (1 if (k // 2) % 2 == 0 else -1)
    if k % 3 == 2:
        c[_position(k + 2, intra)] = _level(2 + (k // 5) % 4, q) * (1 if k % 2 else -1)     # (never a neighbour's first position)
    return c


def dense_block(k, intra):
    """a Full block whose every coefficient row ends in a non-zero LEVEL (columns 6..7), all LEVELs small"""
    rng = np.random.default_rng(1000 + k)
    c = rng.integers(-3, 4, 64).astype(np.int16)
    c[7::8] = 1 + (k + np.arange(8)) % 3
    if intra:
        c[0] = 0
    return c


def wide_block(k, intra, q):
    """a signature plus one LEVEL outside [-512, 511]"""
    c = signature(k, intra, q)
    c[18] = 600 if k % 2 else -700
    return c


def pool_for(mbs, kinds=None):
    """the coefficient pool that goes with finished records: block k of the pool belongs to the k-th coded block in raster
    order (killed blocks have their slot too).  kinds: {(macroblock, block): DENSE / WIDE}.  Returns (coeffs, loud)"""
    kinds = kinds or {}
    pool, loud = [], set()
    for i in range(len(mbs)):
        m = mbs[i]
        intra = int(m["mb_type"]) in INTRA_TYPES
        assert int(m["coeff_index"]) == len(pool)
        for b in range(6):
            if not (int(m["cbp"]) >> b) & 1:
                continue
            k, kind = len(pool), kinds.get((i, b))
            if kind == DENSE:
                pool.append(dense_block(k, intra))
            elif kind == WIDE:
                pool.append(wide_block(k, intra, int(m["quant"])))
            else:
                pool.append(signature(k, intra, int(m["quant"])))
            if kind:
                loud.add(k)
    co = np.array(pool, np.int16).reshape(-1, 64)
    return co, loud


def records_of(w, h, rows):
    """rows: per macroblock row a list of mb() specifications -> (records with coeff_index set, kinds by (macroblock, block))"""
    mbw, mbh = mb_dims(w, h)
    assert len(rows) == mbh and all(len(r) == mbw for r in rows), (w, h, len(rows), [len(r) for r in rows])
    m = np.zeros(mbw * mbh, MB_RECORD_DTYPE)
    kinds, at = {}, 0
    for i, s in enumerate(x for r in rows for x in r):
        m[i]["mb_type"], m[i]["quant"], m[i]["cbp"], m[i]["kill"] = s["t"], s["q"], s["cbp"], s["kill"]
        m[i]["mv"], m[i]["intradc"], m[i]["coeff_index"] = s["mv"], s["dc"], at
        at += popcount(s["cbp"])
        for b, kind in s["kinds"].items():
            assert (s["cbp"] >> b) & 1
            kinds[(i, b)] = kind
    return m, kinds


def picture(table, w, h, rows, picture_type, recode=None, **tag):
    """recode: a function of the finished records that returns the records to use (the bitstream table's quantiser walk);
    the coefficients are made for the records it returns"""
    m, kinds = records_of(w, h, rows)
    if recode:
        m = recode(m)
    co, loud = pool_for(m, kinds)
    return {"table": table, "w": w, "h": h, "mbs": m, "coeffs": co, "picture_type": picture_type, "tag": tag, "loud": loud}


def reference_records(w, h, recode=None):
    """The key frame every P picture of that size is decoded over (a decoder takes a reference in no other way): textured, so
    that a wrong tap or a copy from the wrong place shows, and MID-RANGE -- every pixel within 64..191 (the tests assert it) --
    so that no residual of the tables is hidden by the final clamp.  Returns (mbs, coeffs)."""
    rng = np.random.default_rng(w * 65537 + h + 7)
    mbw, mbh = mb_dims(w, h)
    n = mbw * mbh
    mbs = np.zeros(n, MB_RECORD_DTYPE)
    mbs["mb_type"] = INTRA
    mbs["quant"] = rng.integers(2, 5, n)
    mbs["intradc"] = rng.integers(90, 166, (n, 6))
    mbs["intradc"][mbs["intradc"] == 128] = 129
    mbs["cbp"] = 0x3F
    mbs["coeff_index"] = np.arange(n) * 6
    if recode:
        mbs = recode(mbs)
    co = np.zeros((n * 6, 64), np.int16)
    q = np.repeat(mbs["quant"].astype(np.int64), 6)
    for j in range(3):                                           # up to three small coefficients among the lowest positions
        pos = rng.choice(np.array([1, 2, 8, 9, 10, 16, 17]), n * 6)
        lev = rng.integers(1, 3, n * 6) * rng.choice(np.array([-1, 1]), n * 6)
        lev = np.where(q > 4, np.sign(lev), lev)                 # (a coarse quantiser: +-1 ...
        lev = np.where(q <= 2, 3 * np.sign(lev), lev)            # (the finest ones: enough to show)
        use = (q <= 6) | (j == 0)                                # ... and one coefficient only)
        co[np.flatnonzero(use), pos[use]] = lev[use]
    return mbs, co


# ---------------------------------------------------------------------------------------------------------------
# the anatomy
# ---------------------------------------------------------------------------------------------------------------
def padded_records(pic):
    """state.rs:421-427: macroblocks the picture does not hold are Inter / vector 0 / nothing coded"""
    mbw, mbh = mb_dims(pic["w"], pic["h"])
    out = np.zeros(mbw * mbh, MB_RECORD_DTYPE)
    out["quant"] = 1
    out[:len(pic["mbs"])] = pic["mbs"]
    return out


def has_record(m):
    """sparse record transport: a macroblock that is not coded (Inter, no vector, nothing coded) has no record"""
    return not (int(m["mb_type"]) == INTER and int(m["cbp"]) == 0 and not np.asarray(m["mv"]).any())


def anatomy(pic, sparse=False):
    """what every wave of the picture is: a list of dicts in raster order of (macroblock row, group of 8)"""
    w, h = pic["w"], pic["h"]
    mbw, mbh = mb_dims(w, h)
    mbs = padded_records(pic)
    co = np.asarray(pic["coeffs"], np.int16).reshape(-1, 64)
    has_ref = pic["picture_type"] != PICTURE_I
    kept = np.array([has_record(m) for m in mbs])
    kept_before = np.concatenate([[0], np.cumsum(kept)])
    out = []
    for mby in range(mbh):
        for g in range((mbw + 7) // 8):
            n_valid = min(WAVE_MBS, mbw - 8 * g)
            first = mby * mbw + 8 * g
            recs = [mbs[first + m] for m in range(n_valid)]
            valid = (1 << n_valid) - 1
            act, inter, blocks, moving, uncoded_dc, killed_tasks = 0, 0, {}, [], [], []
            for m, r in enumerate(recs):
                t, cbp, kill = int(r["mb_type"]), int(r["cbp"]), int(r["kill"])
                intra = t in INTRA_TYPES
                if t in INTER_TYPES:
                    inter |= 1 << m
                for vec in range(4):
                    for comp in range(2):
                        if int(r["mv"][vec][comp]):
                            moving.append((m, vec, comp, int(r["mv"][vec][comp])))
                for b in range(6):
                    coded, killed = (cbp >> b) & 1, (kill >> b) & 1
                    dc = int(r["intradc"][b])
                    task = TASK_OF[(m, b)]
                    if (coded and not killed) or (not coded and intra and dc != 0):
                        act |= 1 << task
                        # the block's place in the pool: killed blocks in front of it count
                        levels = co[int(r["coeff_index"]) + popcount(cbp & ((1 << b) - 1))].copy() if coded else np.zeros(64, np.int16)
                        if intra:
                            levels[0] = 0                        # (not a TCOEF: the DC of an intra block is its INTRADC)
                        blocks[task] = levels
                    if intra and not coded:
                        uncoded_dc.append((m, b, dc))
                    if coded and killed:
                        killed_tasks.append(task)
            tasks = [t for t in range(WAVE_TASKS) if (act >> t) & 1]
            n_active = len(tasks)
            n_rounds = (n_active + ROUND_BLOCKS - 1) // ROUND_BLOCKS
            forms = []
            for r in range(n_rounds):
                rb = [blocks[t] for t in tasks[8 * r:8 * r + 8]]
                wide = any(((b < -512) | (b > 511)).any() for b in rb)
                full_rows = len(rb) == 8 and all((b.reshape(8, 8)[:, 6:] != 0).any(axis=1).all() for b in rb)
                forms.append(WIDE if wide else (DENSE if full_rows else GENERAL))
            any_moving = bool(moving)
            quiet = has_ref and act == 0 and valid == 0xff and inter == 0xff
            a = {"mby": mby, "group": g, "n_valid": n_valid, "valid": valid, "act": act, "tasks": tasks, "n_active": n_active,
                 "n_rounds": n_rounds, "last_fill": n_active - 8 * (n_rounds - 1) if n_rounds else 0,
                 "rank": {t: k for k, t in enumerate(tasks)}, "inter": inter, "mc": bool(has_ref and inter),
                 "all_inter": bool(has_ref and inter == valid == 0xff), "any_moving": any_moving, "moving": moving,
                 "static": bool(quiet and not any_moving), "near_static": bool(quiet and any_moving), "forms": forms,
                 "types": [int(r["mb_type"]) for r in recs], "uncoded_dc": uncoded_dc, "killed_tasks": killed_tasks, "has_ref": has_ref,
                 "coded_tasks": [t for t in tasks if (int(recs[task_mb(t)]["cbp"]) >> task_blk(t)) & 1]}
            if sparse:
                mask = sum(1 << m for m in range(n_valid) if kept[first + m])
                a["mask"] = mask
                a["group_word"] = (int(kept_before[first]) << 8 | mask) if mask else 0
                a["copy_by_word"] = bool(has_ref and mask == 0 and valid == 0xff)
            out.append(a)
    return out


def signature_regions(pic, waves=None):
    """[(plane, x, y, pool index)] of the 8x8 blocks whose residual is a signature: active, coded, not loud"""
    mbs = padded_records(pic)
    mbw, _ = mb_dims(pic["w"], pic["h"])
    out = []
    for a in waves or anatomy(pic):
        for t in a["coded_tasks"]:
            r = mbs[a["mby"] * mbw + 8 * a["group"] + task_mb(t)]
            k = int(r["coeff_index"]) + popcount(int(r["cbp"]) & ((1 << task_blk(t)) - 1))
            if k not in pic["loud"]:
                out.append(task_region(t, a["mby"], a["group"]) + (k,))
    return out


def plane_views(pic, planes):
    w, h = pic["w"], pic["h"]
    cw, ch = (w + 1) // 2, (h + 1) // 2
    return [np.asarray(planes[0]).reshape(h, w), np.asarray(planes[1]).reshape(ch, cw), np.asarray(planes[2]).reshape(ch, cw)]


def differing_blocks(pic, got, want):
    """{(plane, x, y)} of the 8x8 blocks in which two sets of planes differ"""
    out = set()
    for k, (g, e) in enumerate(zip(plane_views(pic, got), plane_views(pic, want))):
        ys, xs = np.nonzero(g != e)
        out |= {(k, int(x) & ~7, int(y) & ~7) for x, y in zip(xs, ys)}
    return out


def first_difference(pic, got, want, waves=None):
    """None, or a description of the first differing pixel of three flat planes: which wave, which task, what the wave is"""
    for k, (g, e) in enumerate(zip(plane_views(pic, got), plane_views(pic, want))):
        if g.shape != e.shape:
            return "plane %d: shape %s for %s" % (k, g.shape, e.shape)
        ys, xs = np.nonzero(g != e)
        if len(ys):
            x, y = int(xs[0]), int(ys[0])
            mby, group = (y // 16, x // 128) if k == 0 else (y // 8, x // 64)
            a = [v for v in (waves or anatomy(pic)) if v["mby"] == mby and v["group"] == group][0]
            task = ((y % 16) // 8) * 16 + (x % 128) // 8 if k == 0 else 32 + (k - 1) * 8 + (x % 64) // 8
            return ("%d bytes of plane %d differ; first: got %d, expected %d at (%d, %d): table (%s) %s, wave (row %d, group %d), task %d "
                    "(macroblock %d block %d, %s, rank %s), wave: valid %#x, act %#x (n_active %d), inter %#x, types %s, static %s, "
                    "near static %s, forms %s" % (len(ys), k, g[y, x], e[y, x], x, y, pic["table"], pic["tag"], mby, group, task,
                                                  task_mb(task), task_blk(task), "active" if (a["act"] >> task) & 1 else "idle",
                                                  a["rank"].get(task), a["valid"], a["act"], a["n_active"], a["inter"], a["types"],
                                                  a["static"], a["near_static"], a["forms"]))
    return None


# ---------------------------------------------------------------------------------------------------------------
# (a) every record form
# ---------------------------------------------------------------------------------------------------------------
A_W, A_H = 128, 384                                             # 8 x 24 macroblocks: every macroblock row is one wave


def _form_mb(i, t, cbp, kill):
    q = 1 + i % 31
    if t in INTRA_TYPES:
        return mb(t, cbp, kill, 0, [legal_dc(7 * i + 13 * b) for b in range(6)], q)
    base = np.array([i % 7 - 3, (i // 7) % 5 - 2])
    if t in (INTER4V, INTER4V_Q):
        return mb(t, cbp, kill, base + np.array([[0, 0], [1, 0], [0, 1], [-1, -1]]), 0, q)
    return mb(t, cbp, kill, base, 0, q)


def _forms(intra_only):
    perm = np.random.default_rng(20240).permutation(6 * 64 * 64)
    forms = [(int(f) >> 12, (int(f) >> 6) & 63, int(f) & 63) for f in perm]
    return [f for f in forms if f[0] in INTRA_TYPES] if intra_only else forms


def _table_a(name, picture_type, intra_only):
    forms = _forms(intra_only)
    mbw, mbh = mb_dims(A_W, A_H)
    per = mbw * mbh
    for p in range((len(forms) + per - 1) // per):
        specs = [_form_mb(p * per + j, *forms[(p * per + j) % len(forms)]) for j in range(per)]      # (the last one is filled up)
        yield picture(name, A_W, A_H, [specs[r * mbw:(r + 1) * mbw] for r in range(mbh)], picture_type, picture=p)


def table_a_p():
    return _table_a("a", PICTURE_P, False)


def table_a_i():
    return _table_a("a-I", PICTURE_I, True)


def table_a_dc():
    """uncoded intra blocks with the INTRADC codes at the ends and the middle of the byte (0: nothing; 255: the level 1024)"""
    mbw, mbh = mb_dims(A_W, A_H)
    for picture_type in (PICTURE_P, PICTURE_I):
        specs = []
        for i in range(mbw * mbh):
            if picture_type == PICTURE_P and i % 5 == 4:
                specs.append(mb(INTER, 0, 0, (1, 0)))
                continue
            cbp = (0, 0, 9, 36)[i % 4]
            dc = [legal_dc(i + b) if (cbp >> b) & 1 else DC_EDGE_CODES[(i + b) % 7] for b in range(6)]
            specs.append(mb(INTRA if i % 3 else INTRA_Q, cbp, (i % 8 == 7) * 8, 0, dc, 1 + i % 31))
        yield picture("a-dc", A_W, A_H, [specs[r * mbw:(r + 1) * mbw] for r in range(mbh)], picture_type)


# ---------------------------------------------------------------------------------------------------------------
# (b) every fill
# ---------------------------------------------------------------------------------------------------------------
B_W, B_ROWS = 128, 28
B_KINDS = ("intra", "inter", "mixed")


def b_masks():
    """[(what, value, act mask)]: every count from the low and from the high end, every task alone, every task missing"""
    out = [("low", n, (1 << n) - 1) for n in range(WAVE_TASKS + 1)]
    out += [("high", n, ((1 << n) - 1) << (WAVE_TASKS - n)) for n in range(WAVE_TASKS + 1)]
    out += [("alone", t, 1 << t) for t in range(WAVE_TASKS)]
    out += [("missing", t, ALL_TASKS ^ (1 << t)) for t in range(WAVE_TASKS)]
    return out


def wave_from_mask(act, kind, salt, kinds=None):
    """eight macroblocks whose active tasks are exactly `act`.  An idle block is uncoded or coded and killed (its pool slot
    stays), an active block of an intra macroblock coded or uncoded with a non-zero INTRADC, by turns; kinds: {task: DENSE / WIDE}"""
    kinds = kinds or {}
    out = []
    for m in range(WAVE_MBS):
        intra = kind == "intra" or (kind == "mixed" and (m + salt) % 2 == 0)
        cbp = kill = 0
        dc, bk = [0] * 6, {}
        for b in range(6):
            t = TASK_OF[(m, b)]
            on, turn = (act >> t) & 1, (salt * 7 + t * 3 + (t >> 2)) % 4
            if t in kinds:
                assert on
                cbp |= 1 << b
                bk[b] = kinds[t]
                dc[b] = legal_dc(salt + t)
            elif on and (not intra or turn % 2 == 0):
                cbp |= 1 << b
                dc[b] = legal_dc(salt + t) if intra else 0
            elif on:
                dc[b] = legal_dc(salt + 3 * t)                  # uncoded intra block with a DC: active without a pool slot
            elif turn % 2:
                cbp |= 1 << b                                   # coded and killed: idle, but it holds a pool slot
                kill |= 1 << b
                dc[b] = legal_dc(salt + t) if intra else 0
            elif turn == 2:
                kill |= 1 << b                                  # (a kill bit on a block that is not coded means nothing)
        q = 1 + (salt + 5 * m) % 31
        if intra:
            out.append(mb(INTRA_Q if (m + salt) % 3 == 0 else INTRA, cbp, kill, 0, dc, q, bk))
        else:
            t4 = (m + salt) % 4 == 1
            mv = np.array([[1, -1], [0, 1], [-1, 0], [2, 1]]) if t4 else ((m + salt) % 5 - 2 or 1, (m * 3 + salt) % 3 - 1)
            out.append(mb((INTER4V if t4 else INTER) if (m + salt) % 2 else (INTER4V_Q if t4 else INTER_Q), cbp, kill, mv, 0, q, bk))
    return out


def b_special_waves(kind):
    """the round forms among general rounds: [(tag, act, {task: kind})] -- the active tasks are the n lowest, so rank == task"""
    def low(n):
        return (1 << n) - 1

    def run(first, kind_, n=8):
        return {t: kind_ for t in range(first, first + n)}

    return [
        ("dense@0+partial", low(11), run(0, DENSE)),
        ("dense@1+partial", low(21), run(8, DENSE)),
        ("dense@0,2+partial", low(25), {**run(0, DENSE), **run(16, DENSE)}),
        ("dense-all", low(48), run(0, DENSE, 48)),
        ("wide-among-general", low(20), {11: WIDE}),
        ("wide-in-a-dense-round", low(16), {**run(8, DENSE), 12: WIDE}),
        ("seven-dense-and-one-general", low(16), run(8, DENSE, 7)),
        ("dense-last-full-round", low(16), run(8, DENSE)),
    ]


def table_b(kinds=B_KINDS):
    mbh = B_ROWS
    for kind in kinds:
        masks = b_masks()
        waves = [wave_from_mask(act, kind, i) for i, (_, _, act) in enumerate(masks)]
        n_pictures = (len(waves) + mbh - 1) // mbh
        for p in range(n_pictures):
            rows = [waves[(p * mbh + r) % len(waves)] if p * mbh + r < len(waves) else
                    wave_from_mask(masks[(p * mbh + r) % len(masks)][2], kind, 1000 + r) for r in range(mbh)]
            yield picture("b", B_W, 16 * mbh, rows, PICTURE_I if kind == "intra" else PICTURE_P, kind=kind, picture=p)
        special = b_special_waves(kind)
        rows = [wave_from_mask(act, kind, 50 + i, kinds_) for i, (_, act, kinds_) in enumerate(special)]
        yield picture("b", B_W, 16 * len(rows), rows, PICTURE_I if kind == "intra" else PICTURE_P, kind=kind, picture="forms")


# ---------------------------------------------------------------------------------------------------------------
# (c) wave kinds and widths
# ---------------------------------------------------------------------------------------------------------------
C_MBW = tuple(range(1, 18)) + (24,)
C_NEAR_PICTURES, C_SINGLE_PICTURES = 8, 8


def near_static_wave(n_valid, m, vec, comp, sign):
    out = [mb(INTER4V) for _ in range(n_valid)]
    out[m]["mv"][vec][comp] = sign
    return out


def single_block_wave(n_valid, m, blk, salt):
    out = [mb(INTER) for _ in range(n_valid)]
    out[m] = mb(INTER, 1 << blk, 0, 0, 0, 1 + salt % 31)
    return out


def table_c(widths=C_MBW):
    full_near, full_single = 0, 0
    part = {n: [0, 0] for n in range(1, 8)}
    for mbw in widths:
        w, h = 16 * mbw, 32
        groups = [min(8, mbw - 8 * g) for g in range((mbw + 7) // 8)]
        yield picture("c", w, h, [[mb(INTER) for _ in range(mbw)] for _ in range(2)], PICTURE_P, mbw=mbw, kind="uncoded")
        for j in range(C_NEAR_PICTURES):
            rows = []
            for r in range(2):
                row = []
                for n in groups:
                    if n == 8:
                        v, full_near = full_near % 128, full_near + 1
                        row += near_static_wave(8, v & 7, (v >> 3) & 3, (v >> 5) & 1, 1 if (v >> 6) & 1 else -1)
                    else:
                        k, part[n][0] = part[n][0], part[n][0] + 1
                        row += near_static_wave(n, k % n, (k // n) & 3, (k // (4 * n)) & 1, 1 if (k // (8 * n)) & 1 else -1)
                rows.append(row)
            yield picture("c", w, h, rows, PICTURE_P, mbw=mbw, kind="near", picture=j)
        for j in range(C_SINGLE_PICTURES):
            rows = []
            for r in range(2):
                row = []
                for g, n in enumerate(groups):
                    if n == 8 and (r + g + j) % 2:
                        row += [mb(INTER) for _ in range(8)]     # a static wave beside the active ones
                    elif n == 8:
                        v, full_single = full_single, full_single + 1
                        row += single_block_wave(8, v % 8, (v // 8) % 6, v)
                    else:
                        k, part[n][1] = part[n][1], part[n][1] + 1
                        row += single_block_wave(n, k % n, (k // n) % 6, k)
                rows.append(row)
            yield picture("c", w, h, rows, PICTURE_P, mbw=mbw, kind="single", picture=j)


# ---------------------------------------------------------------------------------------------------------------
# (d) every group word (bitstream path: legal content only)
# ---------------------------------------------------------------------------------------------------------------
D_ROWS, D_PQUANT = 64, 6
D_KINDS = ("vector", "residual", "intra")


def d_size(n):
    return 16 * (8 + n), 16 * D_ROWS


def _d_mb(c):
    kind = D_KINDS[c % 3]
    if kind == "vector":
        return mb(INTER, 0, 0, ((c // 3) % 5 - 2 or 1, (c // 15) % 3 - 1), 0, D_PQUANT)
    if kind == "residual":
        return mb(INTER, (1, 2, 4, 8, 16, 32, 3, 48, 63)[(c // 3) % 9], 0, 0, 0, D_PQUANT)
    cbp = (0, 5, 63, 16)[(c // 3) % 4]
    return mb(INTRA, cbp, 0, 0, [legal_dc(c + 11 * b) for b in range(6)], D_PQUANT)


def table_d(ns=tuple(range(1, 8))):
    """P pictures 16 (8 + n) wide: macroblock row R pairs mask R of the full group with mask (3 R + 1) mod 2^n of the
    partial one (all of them: 3 is odd); a set bit is, by turns, a vector, a residual or an intra macroblock.  The records get
    the quantiser walk DQUANT can express (test_bitstream_e2e.make_codable) before their coefficients are made."""
    from test_bitstream_e2e import make_codable
    for n in ns:
        w, h = d_size(n)
        c = 0
        for p in range(256 // D_ROWS):
            rows = []
            for r in range(D_ROWS):
                R = p * D_ROWS + r
                mask = R | (((3 * R + 1) % (1 << n)) << 8)
                row = []
                for m in range(8 + n):
                    if (mask >> m) & 1:
                        row.append(_d_mb(c))
                        c += 1
                    else:
                        row.append(mb(INTER, q=D_PQUANT))
                rows.append(row)
            yield picture("d", w, h, rows, PICTURE_P, recode=lambda m, s=n * 10 + p: make_codable(m, D_PQUANT, s, 1), n=n, picture=p)


def d_reference_records(n):
    """the key frame of table (d)'s size for n, with a quantiser walk that can be coded"""
    from test_bitstream_e2e import make_codable
    w, h = d_size(n)
    return reference_records(w, h, recode=lambda m: make_codable(m, D_PQUANT, 77 + n, 0))


# ---------------------------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------------------------
class Coverage:
    """what a set of pictures exercises, by the anatomy of their waves.  The conditions are enumerations, not measurements:
    the tables are built so that the tables alone meet them."""

    def __init__(self):
        self.forms = set()              # (a) (picture type, mb_type, cbp, kill)
        self.dc = set()                 # (a) (picture type, INTRADC code of an uncoded intra block)
        self.fill = set()               # (b) (kind, what, value)
        self.rounds = set()             # (b) (n_rounds, fill of the last round)
        self.form_cases = set()         # (b) (what, mc)
        self.ranks = set()              # (b) (task, rank)
        self.c = set()                  # (c)
        self.d_full, self.d_part, self.d_kinds = {}, {}, set()

    def add(self, pic, waves=None, sparse_waves=None):
        waves = waves or anatomy(pic)
        ptype = pic["picture_type"]
        mbs = padded_records(pic)
        table = pic["table"]
        if table.startswith("a"):
            for m in mbs:
                self.forms.add((ptype, int(m["mb_type"]), int(m["cbp"]), int(m["kill"])))
            for a in waves:
                self.dc |= {(ptype, dc) for _, _, dc in a["uncoded_dc"]}
        if table == "b":
            for a in waves:
                self._add_fill(a)
        if table == "c":
            sparse_waves = sparse_waves or anatomy(pic, sparse=True)
            for a, s in zip(waves, sparse_waves):
                self._add_kind(pic, a, s)
        if table == "d":
            sparse_waves = sparse_waves or anatomy(pic, sparse=True)
            n = pic["tag"]["n"]
            for s in sparse_waves:
                (self.d_full if s["n_valid"] == 8 else self.d_part).setdefault(n, set()).add(s["mask"])
                for m, t in enumerate(s["types"]):
                    if (s["mask"] >> m) & 1:
                        r = mbs[s["mby"] * mb_dims(pic["w"], pic["h"])[0] + 8 * s["group"] + m]
                        self.d_kinds.add("intra" if t in INTRA_TYPES else ("residual" if int(r["cbp"]) else "vector"))

    def _add_fill(self, a):
        if a["valid"] != 0xff:
            return
        kind = ("intra" if a["inter"] == 0 and not a["has_ref"] else
                "inter" if a["inter"] == 0xff and a["has_ref"] else "mixed" if a["has_ref"] and a["inter"] else None)
        act, n = a["act"], a["n_active"]
        if kind:
            if act == (1 << n) - 1:
                self.fill.add((kind, "low", n))
            if act == ((1 << n) - 1) << (WAVE_TASKS - n):
                self.fill.add((kind, "high", n))
            if n == 1:
                self.fill.add((kind, "alone", a["tasks"][0]))
            if n == WAVE_TASKS - 1:
                self.fill.add((kind, "missing", [t for t in range(WAVE_TASKS) if not (act >> t) & 1][0]))
        self.rounds.add((a["n_rounds"], a["last_fill"]))
        self.ranks |= set(a["rank"].items())
        f, mc = a["forms"], a["mc"]
        if f and f[0] == DENSE:
            self.form_cases.add(("dense@0", mc))
        if DENSE in f[1:]:
            self.form_cases.add(("dense@later", mc))
        if DENSE in f[:-1] and 0 < a["last_fill"] < 8:
            self.form_cases.add(("dense, then a partial last round", mc))
        if f and all(x == DENSE for x in f) and len(f) == 6:
            self.form_cases.add(("six dense rounds", mc))
        if WIDE in f and GENERAL in f:
            self.form_cases.add(("wide among general", mc))
        if WIDE in f[1:]:
            self.form_cases.add(("wide@later", mc))

    def _add_kind(self, pic, a, s):
        mbw = pic["tag"]["mbw"]
        n = a["n_valid"]
        one = a["moving"][0] if len(a["moving"]) == 1 and abs(a["moving"][0][3]) == 1 else None
        if n == 8:
            if a["static"]:
                self.c.add(("static", mbw))
                if s["copy_by_word"]:
                    self.c.add(("static by an empty group word", mbw))
            if a["near_static"] and one:
                self.c.add(("near static",) + one)
                self.c.add(("near static at width", mbw))
            if a["n_active"] == 1 and not a["any_moving"]:
                self.c.add(("single block", task_mb(a["tasks"][0])))
                self.c.add(("single-bit group word", s["mask"]))
        else:
            assert not a["static"] and not s["copy_by_word"]
            if a["n_active"] == 0 and not a["any_moving"] and a["inter"] == a["valid"]:
                self.c.add(("right edge, uncoded", mbw))
                if s["mask"] == 0:
                    self.c.add(("right edge, empty group word", n))
            if a["n_active"] == 0 and one and a["inter"] == a["valid"]:
                self.c.add(("right edge, near static", n, one[0]))
            if a["n_active"] == 1 and not a["any_moving"]:
                self.c.add(("right edge, single block", n, task_mb(a["tasks"][0])))

    # ---- what is missing from the declared spaces
    def missing_a(self, picture_types=(PICTURE_P, PICTURE_I)):
        want = set()
        if PICTURE_P in picture_types:
            want |= {(PICTURE_P, t, cbp, kill) for t in range(6) for cbp in range(64) for kill in range(64)}
        if PICTURE_I in picture_types:
            want |= {(PICTURE_I, t, cbp, kill) for t in INTRA_TYPES for cbp in range(64) for kill in range(64)}
        return sorted(want - self.forms)[:20]

    def missing_a_dc(self):
        return sorted({(p, c) for p in (PICTURE_P, PICTURE_I) for c in DC_EDGE_CODES} - self.dc)

    def missing_b(self, kinds=B_KINDS):
        want = {(k, what, v) for k in kinds for what, v, _ in b_masks()}
        out = sorted(want - self.fill)[:20]
        # every number of rounds with every fill of the last round, every rank a task can have
        out += sorted(({(0, 0)} | {(r, f) for r in range(1, 7) for f in range(1, 9)}) - self.rounds)
        out += sorted({(t, k) for t in range(WAVE_TASKS) for k in (0, t)} - self.ranks)[:20]
        mcs = {"intra": (False,), "inter": (True,), "mixed": (True,)}
        need = {(what, mc) for k in kinds for mc in mcs[k] for what in (
            "dense@0", "dense@later", "dense, then a partial last round", "six dense rounds", "wide among general", "wide@later")}
        return out + sorted(need - self.form_cases)

    def missing_c(self, widths=C_MBW):
        want = set()
        for mbw in widths:
            if mbw >= 8:
                want |= {("static", mbw), ("static by an empty group word", mbw), ("near static at width", mbw)}
            n = mbw % 8
            if n:
                want |= {("right edge, uncoded", mbw), ("right edge, empty group word", n)}
                want |= {("right edge, near static", n, m) for m in range(n)}
                want |= {("right edge, single block", n, m) for m in range(n)}
        if any(mbw >= 8 for mbw in widths) and set(widths) >= set(C_MBW):
            want |= {("near static", m, vec, comp, sign) for m in range(8) for vec in range(4) for comp in range(2) for sign in (-1, 1)}
            want |= {("single block", m) for m in range(8)} | {("single-bit group word", 1 << m) for m in range(8)}
        return sorted(want - self.c, key=str)

    def missing_d(self, ns=tuple(range(1, 8))):
        out = []
        for n in ns:
            out += [(n, "full", m) for m in sorted(set(range(256)) - self.d_full.get(n, set()))[:8]]
            out += [(n, "partial", m) for m in sorted(set(range(1 << n)) - self.d_part.get(n, set()))[:8]]
        return out + sorted(set(D_KINDS) - self.d_kinds)
