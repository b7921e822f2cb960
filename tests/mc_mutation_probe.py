"""Decodes the motion-compensation mutation pictures -- table (d) (whole-wave integer vectors) and table (f) (every pair
of tap sums, as flat 8x8 blocks) of tests/mc_cases.py -- with whichever build of the library H263MI_LIB names and saves
every plane.  Run as a child process by tests/test_gpu_mutation.py: a process can load one build of the library only.

Also here, because both sides of that test need them: the numpy MODELS of the two mutations (csrc/mutants.h), which
predict every byte a mutant build must produce.
  blend      blend_rows without the `^ (both & dm)` exclusion: a (1/2, 1/2) pixel with tap sums a + s = 2 Ha + la and
             b + t = 2 Hb + lb comes out as ((Ha + Hb + 1) >> 1) + (la & lb): one too many where both dropped bits are
             set and Ha + Hb is odd
  intborder  a border lane of a wave whose vectors are all integer keeps the 12 bytes it loaded at the border window
             (recon_kernel.inl: border_window) and shifts them by u & 3 like an inside lane: pixel i of a row is
             window byte (u & 3) + i instead of the clamped tap
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "h263-rs_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import mc_cases as mc  # noqa: E402


def pictures_d():
    return list(mc.table_d())


def pictures_f():
    """table (f) at the size of its flat-block reference"""
    return list(mc.table_f(8 * mc.F_LUMA))


# ---------------------------------------------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------------------------------------------
def _plane_inputs(pic, ref):
    """per plane: (reference plane 2-D, per-block arrays of the classifier, predicted mask), luma then Cb, Cr"""
    mbs, inter, mv, (Y, Cc) = mc.Coverage.planes(pic)
    assert not mbs["cbp"].any(), "the models cover pictures without residuals"
    w, h = pic["w"], pic["h"]
    cw, ch = (w + 1) // 2, (h + 1) // 2
    return mbs, inter, [(np.asarray(ref[0]).reshape(h, w), Y), (np.asarray(ref[1]).reshape(ch, cw), Cc),
                        (np.asarray(ref[2]).reshape(ch, cw), Cc)]


def _grid(P, name, mbw, mbh):
    """a per-block array of the classifier as a 2-D grid of blocks"""
    a = P[name]
    if a.shape[1] == 4:                                         # luma: [mb, block] -> [2 mbh, 2 mbw]
        return a.reshape(mbh, mbw, 2, 2).transpose(0, 2, 1, 3).reshape(2 * mbh, 2 * mbw)
    return a.reshape(mbh, mbw)


def _per_pixel(a):
    return np.repeat(np.repeat(a, 8, axis=0), 8, axis=1)


def _taps(plane, mvx, mvy):
    h, w = plane.shape
    dx, ix, dy, iy = _per_pixel(mvx >> 1), _per_pixel(mvx & 1), _per_pixel(mvy >> 1), _per_pixel(mvy & 1)
    us = np.arange(dx.shape[1])[None, :] + dx
    vs = np.arange(dx.shape[0])[:, None] + dy
    p = plane.astype(np.int32)

    def tap(du, dv):
        return p[np.clip(vs + dv, 0, h - 1), np.clip(us + du, 0, w - 1)]

    return tap(0, 0), tap(1, 0), tap(0, 1), tap(1, 1), ix, iy


def model_blend(pic, ref, want):
    """the planes the blend mutant must produce: the oracle's (`want`) plus one in the (1/2, 1/2) pixels whose two dropped
    bits are both set while Ha + Hb is odd (never a carry: la = 1 means Ha <= 254, and an odd sum rounds to at most 254)"""
    mbw, mbh = mc.mb_dims(pic["w"], pic["h"])
    mbs, inter, planes = _plane_inputs(pic, ref)
    out = []
    for k, (plane, P) in enumerate(planes):
        ph, pw = plane.shape
        mvx, mvy, pred = (_grid(P, n, mbw, mbh) for n in ("mvx", "mvy", "pred"))
        a, s, b, t, ix, iy = _taps(plane, mvx, mvy)
        ha, la, hb, lb = (a + s) >> 1, (a + s) & 1, (b + t) >> 1, (b + t) & 1
        extra = (ix & iy & la & lb & ((ha + hb) & 1)) * _per_pixel(pred)
        out.append((np.asarray(want[k]).reshape(ph, pw) + extra[:ph, :pw]).astype(np.uint8).ravel())
    return tuple(out)


def integer_waves(pic):
    """per plane kind: bool[mbh, mbw], set for the macroblocks of a wave that takes the integer short cut there"""
    mbs, inter, mv, planes = mc.Coverage.planes(pic)
    mbw, mbh = mc.mb_dims(pic["w"], pic["h"])
    out = {}
    for P in planes:
        odd = (((P["mvx"] | P["mvy"]) & 1) != 0).any(axis=1).reshape(mbh, mbw)
        m = np.zeros((mbh, mbw), bool)
        for x0 in range(0, mbw, 8):
            m[:, x0:x0 + 8] = ~odd[:, x0:x0 + 8].any(axis=1, keepdims=True)
        # (a wave nothing is predicted in, or one that only copies, never gets to the branch: no border lane there either way)
        out[P["kind"]] = m
    return out


def model_intborder(pic, ref, want):
    """the planes the integer-border mutant must produce: the oracle's (`want`), except in the blocks of border lanes of
    all-integer waves"""
    mbw, mbh = mc.mb_dims(pic["w"], pic["h"])
    mbs, inter, planes = _plane_inputs(pic, ref)
    waves = integer_waves(pic)
    out = []
    for k, (plane, P) in enumerate(planes):
        ph, pw = plane.shape
        got = np.asarray(want[k]).reshape(ph, pw).copy()
        mvx, mvy, pred, px, py = (_grid(P, n, mbw, mbh) for n in ("mvx", "mvy", "pred", "px", "py"))
        per_mb = 2 if P["kind"] == "Y" else 1
        in_wave = np.repeat(np.repeat(waves[P["kind"]], per_mb, axis=0), per_mb, axis=1)
        u, v = px + (mvx >> 1), py + (mvy >> 1)
        border = pred & in_wave & ~((u >= 0) & (u <= pw - 8))
        for by, bx in np.argwhere(border):
            uu, vv, x0, y0 = int(u[by, bx]), int(v[by, bx]), int(px[by, bx]), int(py[by, bx])
            ub = 0 if (uu < 0 or ((pw - 9) & ~3) < 0) else (pw - 9) & ~3                       # border_window
            for j in range(8):
                for i in range(8):
                    if x0 + i < pw and y0 + j < ph:
                        src = ub + (uu & 3) + i
                        assert src < pw, "the model knows the picture's bytes only"
                        got[y0 + j, x0 + i] = plane[min(max(vv + j, 0), ph - 1), src]
        out.append(got.ravel())
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------
# the child: decode everything with the library under test
# ---------------------------------------------------------------------------------------------------------------
def decode_all():
    """{name: (y, cb, cr)} of every probe picture, each over its freshly installed reference"""
    import h263mi
    out = {}
    st = h263mi.H263State()
    for k, pic in enumerate(pictures_d()):
        mbs, co = mc.reference_records(pic["w"], pic["h"])
        st.submit_picture(pic["w"], pic["h"], mbs, co, h263mi.PICTURE_I)
        st.submit_picture(pic["w"], pic["h"], pic["mbs"], pic["coeffs"], h263mi.PICTURE_P, temporal_reference=1)
        out["d%03d" % k] = st.get_last_picture().as_yuv()
    st.close()
    w, h, intra, push, co = mc.f_blocks_reference()
    st = h263mi.H263State()
    for k, pic in enumerate(pictures_f()):
        st.submit_picture(w, h, intra, mc.NO_COEFFS, h263mi.PICTURE_I)
        st.submit_picture(w, h, push, co, h263mi.PICTURE_P, temporal_reference=1)
        st.submit_picture(w, h, pic["mbs"], pic["coeffs"], h263mi.PICTURE_P, temporal_reference=2)
        out["f%d" % k] = st.get_last_picture().as_yuv()
    st.close()
    return out


if __name__ == "__main__":
    res = decode_all()
    np.savez(sys.argv[1], **{"%s_%d" % (name, i): p for name, planes in res.items() for i, p in enumerate(planes)})
