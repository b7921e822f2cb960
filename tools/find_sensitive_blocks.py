#!/usr/bin/env python3
"""Finds 8x8 blocks on which an arithmetic MUTATION of the IDCT changes a reconstructed pixel, with the FPU-free
soft-float model (oracle/softfloat_idct.py), and writes them to tests/golden/idct_sensitive_blocks.json.

The reference IDCT (idct.rs:52-65) rounds every product and every partial sum to binary32, in the order of the
frequency index.  Two implementations a GPU port is tempted by give slightly different sums: fusing the multiply
into the add (v_fma_f32 / v_pk_fma_f32 / MFMA: -ffp-contract=fast) and summing the eight products as a tree.  The
final `(v / 4 + signum(v) / 2) as i16` hides almost all of those differences; this search finds the blocks where it
does not, so that tests/test_gpu_mutation.py can prove that the GPU parity suite would catch either mutation.

Blocks are inter blocks (LEVELs + quantiser, dequantised per rle.rs:130-133) meant to be decoded over a flat
prediction of 128, so residuals in [-128, 127] are visible in the output.

usage: python tools/find_sensitive_blocks.py [n_blocks=400000] [seed=1]     (several minutes on 8 cores)
       python tools/find_sensitive_blocks.py --kinds [seed=1]                (writes idct_sensitive_forms.json)

--kinds searches, per KIND of block, for blocks of that kind alone -- the kinds are the shapes that steer a reconstruction
round of the port into another stretch of machine code: the extent of the truncated sums (corner2 /
corner4 / corner6), the one-transform classes (vert, horiz), the dense round, and intra blocks (the DC is the INTRADC level,
the pixel is clamp(residual, 0, 255) with no prediction underneath).  tests/idct_form_cases.py places them.
"""
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import softfloat_idct as sf  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "idct_sensitive_blocks.json")


def make_blocks(rng, n):
    levels = np.zeros((n, 64), np.int64)
    quant = rng.integers(1, 32, n)
    for b in range(n):
        k = int(rng.integers(2, 14))
        pos = rng.choice(64, k, replace=False)
        amp = int(rng.choice([3, 8, 20, 40]))
        lv = rng.integers(-amp, amp + 1, k)
        lv[lv == 0] = 1
        levels[b, pos] = lv
        # make sure it is a Full block: something off the first row and off the first column
        if not (levels[b].reshape(8, 8)[1:, 1:] != 0).any():
            levels[b, 9 + int(rng.integers(0, 7))] = 1 + int(rng.integers(0, amp))
    return levels, quant


def dequant_all(levels, quant):
    q = quant[:, None]
    m = q * (2 * np.abs(levels) + 1) - (q % 2 == 0)
    return np.clip(np.where(levels > 0, m, np.where(levels < 0, -m, 0)), -2048, 2047)


def scan(args):
    seed, n = args
    rng = np.random.default_rng(seed)
    levels, quant = make_blocks(rng, n)
    co = dequant_all(levels, quant)
    res, out = sf.vfull_residual(co)
    # t = v / 4 + signum(v) / 2 in binary32; near-tie = within 6 ulp of an integer, |t| in (1, 127)
    quarter = np.full(out.shape, sf.QUARTER, np.uint32)
    t = sf.vf32_add(sf.vf32_mul(out, quarter), (out & np.uint32(0x80000000)) | np.uint32(sf.HALF))
    e = ((t >> np.uint32(23)) & np.uint32(0xFF)).astype(np.int64)
    m = ((t & np.uint32(0x7FFFFF)) | np.uint32(0x800000)).astype(np.int64)
    fb = np.clip(150 - e, 1, 30)
    frac = m & ((np.int64(1) << fb) - 1)
    dist = np.minimum(frac, (np.int64(1) << fb) - frac)
    near = (dist <= 6) & (e >= 127) & (e <= 133)
    found = []
    for b in np.flatnonzero(near.any(axis=(1, 2))):
        c = [int(x) for x in co[b]]
        ref = sf.block_residual(c, "reference")
        assert ref == res[b].tolist()
        entry = None
        for mode in ("fma", "pairwise"):
            mut = sf.block_residual(c, mode)
            diff = [(y, x) for y in range(8) for x in range(8) if mut[y][x] != ref[y][x] and -128 <= ref[y][x] <= 127 and
                    -128 <= mut[y][x] <= 127]
            if diff:
                entry = entry or {"quant": int(quant[b]), "levels": [int(v) for v in levels[b]], "residual": ref, "detects": {}}
                entry["detects"][mode] = [[y, x, mut[y][x]] for y, x in diff]
        if entry:
            found.append(entry)
    return found


# ---------------------------------------------------------------------------------------------------------------
# --kinds
# ---------------------------------------------------------------------------------------------------------------
OUT_KINDS = os.path.join(ROOT, "tests", "golden", "idct_sensitive_forms.json")
KINDS = ("corner2", "corner4", "corner6", "vert", "horiz", "dense", "intra_full", "intra_dense")
MUTATIONS = ("fma", "pairwise")
# the pairs the model shows no mutation can change, with the reason (exempt in every test)
EXEMPT = {("corner2", "pairwise"): "two terms per sum: the balanced tree (p0 + p1) + (0 + 0) + ... IS the sequential sum"}
# the six blocks of a macroblock share its quantiser: few quantisers, so that tests can fill macroblocks with blocks of a kind
KIND_QUANTS = (1, 2, 3, 5, 8, 13)
DENSE_QUANTS = (1, 2, 3)
PER_PAIR, CHUNK, BATCH, MAX_BATCHES = 10, 4000, 8, 150


def is_intra(kind):
    return kind.startswith("intra")


def intradc_level(code):
    """block.rs / rle.rs:117-121: the code 255 stands for the level 1024, every other one for 8 x itself"""
    return 1024 if code == 255 else 8 * code


def make_kind_blocks(rng, kind, n):
    """-> (LEVELs [n, 64] raster, quantisers [n], INTRADC codes [n] (0: an inter block))"""
    levels = np.zeros((n, 64), np.int64)
    dense = kind in ("dense", "intra_dense")
    quant = rng.choice(np.array(DENSE_QUANTS if dense else KIND_QUANTS), n)
    code = rng.integers(64, 192, n) if is_intra(kind) else np.zeros(n, np.int64)
    code[code == 128] = 129
    for b in range(n):
        g = levels[b].reshape(8, 8)
        if dense:
            amp = int(rng.integers(1, 4))
            lv = rng.integers(-amp, amp + 1, (8, 8))
            g[:] = np.where(rng.random((8, 8)) < rng.choice([0.2, 0.4, 0.8]), lv, 0)
            for r in range(8):                               # the dense-round condition: every row ends in its last pair
                if not g[r, 6:].any():
                    g[r, 6 + int(rng.integers(0, 2))] = int(rng.choice([-1, 1])) * int(rng.integers(1, amp + 1))
        elif kind in ("vert", "horiz"):
            k = int(rng.integers(2, 9))
            pos = rng.choice(8, k, replace=False)
            amp = int(rng.choice([3, 8, 20, 40]))
            lv = rng.integers(-amp, amp + 1, k)
            lv[lv == 0] = 1
            line = np.zeros(8, np.int64)
            line[pos] = lv
            if not line[1:].any():
                line[1 + int(rng.integers(0, 7))] = 1 + int(rng.integers(0, amp))
            if kind == "vert":
                g[:, 0] = line
            else:
                g[0, :] = line
        else:
            c = int(kind[-1]) if kind.startswith("corner") else 8
            k = int(rng.integers(2, min(14, c * c) + 1))
            pos = rng.choice(c * c, k, replace=False)
            amp = int(rng.choice([3, 8, 20, 40]))
            lv = rng.integers(-amp, amp + 1, k)
            lv[lv == 0] = 1
            g[pos // c, pos % c] = lv
            if kind.startswith("corner"):
                # the block alone makes a round of c x c: something in row c - 1, something in the last pair of columns
                if not g[c - 1, :c].any():
                    g[c - 1, int(rng.integers(0, c))] = 1 + int(rng.integers(0, amp))
                if not g[:c, max(1, c - 2):c].any():
                    g[int(rng.integers(0, c)), c - 1] = -1 - int(rng.integers(0, amp))
            # a Full block: something off the first row and something off the first column
            if not g[1:, :].any() or not g[:, 1:].any():
                g[1, 1] = 1 + int(rng.integers(0, amp))
        if is_intra(kind):
            g[0, 0] = 0                                      # (not a TCOEF: the DC of an intra block is its INTRADC)
            if not g[1:, :].any() or not g[:, 1:].any():
                g[1, 1] = 1
    return levels, quant, code


def kind_of(levels, intra):
    """the kinds a block of LEVELs (raster) belongs to -- what make_kind_blocks promises, for the consistency tests"""
    g = np.asarray(levels).reshape(8, 8) != 0
    if intra:
        g = g.copy()
        g[0, 0] = True                                       # (a legal INTRADC is never 0)
    horiz, vert = not g[1:, :].any(), not g[:, 1:].any()
    if horiz or vert:
        return set() if horiz and vert else {"horiz" if horiz else "vert"}
    out = {"intra_full"} if intra else set()
    if g[:, 6:].any(axis=1).all():
        out.add("intra_dense" if intra else "dense")
    if not intra:
        for c in (2, 4, 6):
            if not g[c:, :].any() and not g[:, c:].any() and g[c - 1, :].any() and g[:, max(1, c - 2):c].any():
                out.add("corner%d" % c)
    return out


def coefficients(levels, quant, code):
    co = dequant_all(levels, quant)
    return np.where(np.arange(64)[None, :] == 0, np.where(code[:, None] > 0, np.where(code[:, None] == 255, 1024, 8 * code[:, None]), co), co)


def scan_kind(args):
    kind, seed, n = args
    rng = np.random.default_rng(seed)
    levels, quant, code = make_kind_blocks(rng, kind, n)
    co = coefficients(levels, quant, code)
    if kind in ("vert", "horiz"):
        res, out = sf.vline_residual(co[:, 0::8] if kind == "vert" else co[:, :8])
        x = sf.vf32_mul(out, np.full(out.shape, sf.BASIS_BITS[0][0], np.uint32))
    else:
        res, out = sf.vfull_residual(co)
        x = out
    quarter = np.full(out.shape, sf.QUARTER, np.uint32)
    t = sf.vf32_add(sf.vf32_mul(x, quarter), (out & np.uint32(0x80000000)) | np.uint32(sf.HALF))
    e = ((t >> np.uint32(23)) & np.uint32(0xFF)).astype(np.int64)
    m = ((t & np.uint32(0x7FFFFF)) | np.uint32(0x800000)).astype(np.int64)
    fb = np.clip(150 - e, 1, 30)
    frac = m & ((np.int64(1) << fb) - 1)
    dist = np.minimum(frac, (np.int64(1) << fb) - frac)
    near = (dist <= 6) & (e >= 127) & (e <= (134 if is_intra(kind) else 133))
    lo, hi = (1, 254) if is_intra(kind) else (-128, 127)     # visible: over a prediction of 128 / as the pixel itself
    found = []
    for b in np.flatnonzero(near.reshape(n, -1).any(axis=1)):
        c = [int(v) for v in co[b]]
        ref = sf.block_residual(c, "reference")
        want = res[b].tolist()
        if kind == "vert":
            want = [[v] * 8 for v in want]
        elif kind == "horiz":
            want = [want] * 8
        assert ref == want and kind in kind_of(levels[b], is_intra(kind)), (kind, seed, int(b))
        entry = None
        for mode in MUTATIONS:
            mut = sf.block_residual(c, mode)
            diff = [(y, xx) for y in range(8) for xx in range(8) if mut[y][xx] != ref[y][xx] and lo <= ref[y][xx] <= hi and
                    lo <= mut[y][xx] <= hi]
            if diff:
                entry = entry or {"kind": kind, "quant": int(quant[b]), "levels": [int(v) for v in levels[b]], "residual": ref,
                                  "detects": {}}
                if is_intra(kind):
                    entry["intradc"] = int(code[b])
                entry["detects"][mode] = [[y, xx, mut[y][xx]] for y, xx in diff]
        if entry:
            found.append(entry)
    return found


def main_kinds(seed):
    blocks, searched = [], {}
    with ProcessPoolExecutor(8) as ex:
        for ki, kind in enumerate(KINDS):
            need = [mu for mu in MUTATIONS if (kind, mu) not in EXEMPT]
            found, batches = [], 0
            while batches < MAX_BATCHES and any(sum(mu in f["detects"] for f in found) < PER_PAIR for mu in need):
                jobs = [(kind, seed * 10000000 + ki * 100000 + batches * BATCH + i, CHUNK) for i in range(BATCH)]
                for part in ex.map(scan_kind, jobs):
                    found += part
                batches += 1
                print("%s: %d blocks searched, %s" % (kind, batches * BATCH * CHUNK,
                                                      {mu: sum(mu in f["detects"] for f in found) for mu in MUTATIONS}), flush=True)
            searched[kind] = batches * BATCH * CHUNK
            keep = []
            for mu in need:
                have = [f for f in found if mu in f["detects"]]
                assert len(have) >= 8, "the budget (MAX_BATCHES) is too small for %s / %s: %d found" % (kind, mu, len(have))
                keep += [f for f in have[:PER_PAIR] if f not in keep]
            for mu, why in ((m_, w_) for (k_, m_), w_ in EXEMPT.items() if k_ == kind):
                assert not any(mu in f["detects"] for f in found), "%s / %s is exempt because %s -- yet the model found one" % (kind, mu, why)
            blocks += keep
    doc = {"note": "Blocks of one KIND each (raster-order LEVELs + quantiser; intra blocks: + the INTRADC code, LEVEL 0 unused) on "
                   "which a fused multiply-add (`fma`) or a pairwise summation (`pairwise`) in idct_1d changes the clipped residual "
                   "of at least one pixel.  Layout as idct_sensitive_blocks.json; an inter block's difference counts where both "
                   "residuals are in -128..127 (visible over a prediction of 128), an intra block's where both are in 1..254 "
                   "(the pixel is clamp(residual, 0, 255)).  Kinds: corner2/4/6 = Full, every LEVEL inside the top-left c x c; "
                   "vert / horiz = first column / first row only; dense = every coefficient row has a LEVEL in columns 6..7; "
                   "intra_full / intra_dense = the same with the DC from INTRADC.  EXEMPT (the model shows the mutation cannot "
                   "change anything): %s.  Found by tools/find_sensitive_blocks.py --kinds with the FPU-free soft-float model "
                   "(oracle/softfloat_idct.py), seed %d, quantisers %s (dense kinds %s), random blocks searched per kind: %s."
                   % ("; ".join("%s / %s -- %s" % (k_, m_, w_) for (k_, m_), w_ in EXEMPT.items()), seed, list(KIND_QUANTS),
                      list(DENSE_QUANTS), searched),
           "exempt": [[k_, m_] for k_, m_ in EXEMPT],
           "blocks": blocks}
    json.dump(doc, open(OUT_KINDS, "w"), separators=(",", ":"))
    print("wrote %s: %d blocks" % (OUT_KINDS, len(blocks)))
    for kind in KINDS:
        print("  %-12s %s" % (kind, {mu: sum(mu in f["detects"] for f in blocks if f["kind"] == kind) for mu in MUTATIONS}))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--kinds":
        return main_kinds(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 400000
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    chunk = 5000
    jobs = [(seed * 100000 + i, chunk) for i in range(n // chunk)]
    found = []
    with ProcessPoolExecutor(8) as ex:
        for part in ex.map(scan, jobs):
            found += part
            print("blocks so far: %d (fma %d, pairwise %d)" % (len(found), sum("fma" in f["detects"] for f in found),
                                                                 sum("pairwise" in f["detects"] for f in found)), flush=True)
    fma = [f for f in found if "fma" in f["detects"]][:48]
    pw = [f for f in found if "pairwise" in f["detects"] and f not in fma][:48]
    doc = {"note": "Full-class inter blocks (raster-order LEVELs + quantiser) on which a fused multiply-add (`fma`) or a "
                   "pairwise summation (`pairwise`) in idct_1d changes the clipped residual of at least one pixel; "
                   "`residual`[y][x] is the reference arithmetic's (idct.rs:52-65, 171-196), `detects`[mutation] lists "
                   "[y, x, mutated residual].  Found by tools/find_sensitive_blocks.py with the FPU-free soft-float "
                   "model (oracle/softfloat_idct.py), seed %d, %d random blocks." % (seed, n),
           "blocks": fma + pw}
    json.dump(doc, open(OUT, "w"), separators=(",", ":"))
    print("wrote %s: %d blocks (%d detect fma, %d detect pairwise)" % (OUT, len(doc["blocks"]),
          sum("fma" in f["detects"] for f in doc["blocks"]), sum("pairwise" in f["detects"] for f in doc["blocks"])))


if __name__ == "__main__":
    main()
