"""Bilinear and bicubic resampling (h263mi_filter): h263mi_filter_taps -- a pure host function, so all of this runs without a
device -- against the restatement in Python floats (filter_ref.py); the 32-bit bound of every table row; every refusal; and the
restatement itself against Pillow, whose Image.resize on a mode-RGB image is the definition."""
import ctypes as C

import numpy as np
import pytest

import filter_cases as fc
import filter_ref as ref
import h263mi

BAD = h263mi.ERR_INVALID_ARGUMENT


def _axes():
    """(in, out) of every case's two axes"""
    out = set()
    for name in fc.CASES:
        (_, _, sw, sh), (_, _, dw, dh) = fc.rects(name)
        out |= {(sw, dw), (sh, dh)}
    return sorted(out)


def _same_taps(kind, n_in, n_out):
    ks, first, count, coeffs = h263mi.filter_taps(kind, n_in, n_out)
    wks, wfirst, wcount, wcoeffs = ref.taps(kind, n_in, n_out)
    assert ks == wks, (kind, n_in, n_out, ks, wks)
    assert (first == wfirst).all() and (count == wcount).all() and (coeffs == wcoeffs).all(), (kind, n_in, n_out)
    return coeffs


def _bound(coeffs):
    """255 * sum |coeff| + 2^21 < 2^31 for every row: int32 holds every sum of a pass"""
    worst = int(np.abs(coeffs.astype(np.int64)).sum(axis=1).max())
    assert 255 * worst + (1 << 21) < 1 << 31, worst


@pytest.mark.parametrize("kind", fc.KINDS, ids=fc.KIND_IDS)
def test_taps_match_the_restatement_at_the_cases_axes(kind):
    for n_in, n_out in _axes():
        _bound(_same_taps(kind, n_in, n_out))


@pytest.mark.parametrize("kind", fc.KINDS, ids=fc.KIND_IDS)
def test_taps_match_the_restatement_1_to_64(kind):
    for n_in in range(1, 65):
        for n_out in range(1, 65):
            coeffs = _same_taps(kind, n_in, n_out)
            _bound(coeffs)
            # the weights of a position sum to one, but for the roundings of its taps
            assert (np.abs(coeffs.astype(np.int64).sum(axis=1) - (1 << 22)) <= coeffs.shape[1]).all(), (n_in, n_out)


@pytest.mark.parametrize("kind", fc.KINDS, ids=fc.KIND_IDS)
@pytest.mark.parametrize("n_in,n_out", [(65535, 1), (1, 65535), (65535, 65535), (1920, 224), (1080, 224)])
def test_the_32_bit_bound_at_the_largest_sizes(kind, n_in, n_out):
    ks, first, count, coeffs = h263mi.filter_taps(kind, n_in, n_out)
    _bound(coeffs)
    assert (count <= ks).all() and (first.astype(np.int64) + count <= n_in).all() and (count >= 1).all()
    if n_in == 65535 and n_out == 1:
        assert ks == 2 * int(np.ceil((2.0 if kind == ref.BICUBIC else 1.0) * 65535)) + 1 and count[0] == 65535


def test_every_refusal():
    L = h263mi.lib()
    ks = C.c_uint32(77)
    first, count = np.zeros(8, np.uint32), np.zeros(8, np.uint32)
    coeffs = np.zeros(8 * 16, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    good = lambda kind, n_in, n_out, cap: L.h263mi_filter_taps(kind, n_in, n_out, C.byref(ks), p(first), p(count), p(coeffs), cap)
    assert good(ref.BILINEAR, 16, 8, coeffs.size) == h263mi.OK and ks.value == 5
    assert L.h263mi_filter_taps(ref.BILINEAR, 16, 8, None, None, None, None, 0) == BAD            # nowhere to answer
    assert L.h263mi_filter_taps(ref.BICUBIC, 16, 8, C.byref(ks), None, None, None, 0) == h263mi.OK and ks.value == 9   # the size alone
    for kind in (ref.AREA, 3, 255):                                                                # AREA has no taps
        assert good(kind, 16, 8, coeffs.size) == BAD and ref.taps(kind, 16, 8) is None
    for n_in, n_out in ((0, 8), (16, 0), (65536, 8), (16, 65536)):
        assert good(ref.BILINEAR, n_in, n_out, coeffs.size) == BAD and ref.taps(ref.BILINEAR, n_in, n_out) is None
    assert good(ref.BILINEAR, 16, 8, 8 * 5 - 1) == BAD and good(ref.BILINEAR, 16, 8, 8 * 5) == h263mi.OK
    assert L.h263mi_filter_taps(ref.BILINEAR, 16, 8, C.byref(ks), None, p(count), p(coeffs), coeffs.size) == BAD
    assert L.h263mi_filter_taps(ref.BILINEAR, 16, 8, C.byref(ks), p(first), None, p(coeffs), coeffs.size) == BAD
    # a refused call writes nothing
    coeffs[:] = 12345
    assert good(ref.BILINEAR, 16, 8, 3) == BAD and (coeffs == 12345).all()
    # the entry points that take a filter refuse a missing handle before anything else (no device is needed to say so)
    r, _ = h263mi.make_rgba_resize(8, 8)
    t = h263mi.make_tensor_out(8, 8, h263mi.TENSOR_F32)
    f = h263mi.make_filter(ref.BICUBIC)
    out = np.zeros(8 * 8 * 4 * 3, np.uint8)
    assert L.h263mi_batch_set_rgba_resize_filtered(None, C.byref(r), None, C.byref(f)) == BAD
    assert L.h263mi_batch_set_tensor_output_filtered(None, C.byref(t), None, C.byref(f)) == BAD
    assert L.h263mi_mixed_set_rgba_resize_filtered(None, C.byref(r), None, C.byref(f)) == BAD
    assert L.h263mi_mixed_set_tensor_output_filtered(None, C.byref(t), None, C.byref(f)) == BAD
    assert L.h263mi_render_rgba_resize_filtered(None, 0, C.byref(r), None, C.byref(f), p(out)) == BAD
    assert L.h263mi_render_tensor_filtered(None, 0, C.byref(t), None, C.byref(f), p(out)) == BAD


def test_struct_layout():
    assert C.sizeof(h263mi.Filter) == 8 and h263mi.Filter.reserved.offset == 1
    assert (h263mi.FILTER_AREA, h263mi.FILTER_BILINEAR, h263mi.FILTER_BICUBIC) == (ref.AREA, ref.BILINEAR, ref.BICUBIC)


def test_an_intra_picture_reaches_the_clamp_in_both_passes():
    """the pictures of the device tests (recgen.intra_picture through the oracle, deblocked, BT.601) leave 0..255 on both sides in
    both passes of the cubic, and hold pixels where one rounding is not two: those tests can tell a clamp from a mask"""
    import recgen
    from oracle import oracle as orc
    want = {"h_clamp_0", "h_clamp_255", "v_clamp_0", "v_clamp_255", "single_rounding_differs", "mask_differs"}
    for (w, h), name in ((fc.QCIF, "qcif_224"), (fc.CIF, "cif_50x37")):
        mbs, co = recgen.intra_picture(w, h, seed=w + 5)
        rc, planes = orc.decode_picture(w, h, mbs, co, None)
        assert rc == 0
        cw = (w + 1) // 2
        planes = tuple(orc.deblock(p, pw, 7) for p, pw in zip(planes, (w, cw, cw)))
        full = np.asarray(orc.yuv420_to_rgba(*planes, w), np.uint8).reshape(h, w, 4)
        assert want <= fc.content_hazards(name, ref.BICUBIC, full), (name, fc.content_hazards(name, ref.BICUBIC, full))


# ---------------------------------------------------------------------------------------------
# the restatement against Pillow
# ---------------------------------------------------------------------------------------------
def _pil_filter(Image, kind):
    resampling = getattr(Image, "Resampling", Image)
    return resampling.BILINEAR if kind == ref.BILINEAR else resampling.BICUBIC


@pytest.mark.parametrize("kind", fc.KINDS, ids=fc.KIND_IDS)
@pytest.mark.parametrize("name", list(fc.CASES))
def test_restatement_is_pillow_crop_then_resize(name, kind):
    Image = pytest.importorskip("PIL.Image")
    size, (ow, oh), _, _, _ = fc.CASES[name]
    (sx, sy, sw, sh), (dx, dy, dw, dh) = fc.rects(name)
    full = fc.picture(size, 0)
    im = Image.fromarray(np.ascontiguousarray(full[:, :, :3]), "RGB")
    # the unframed sizes of the case: the whole picture to W' x H'
    whole = np.asarray(im.resize((ow, oh), _pil_filter(Image, kind)))
    assert (ref.resize(full[:, :, :3], ow, oh, kind) == whole).all()
    # the framed form: the window cropped, then resized (its own edges end the taps), pasted into the pad colour
    want = np.empty((oh, ow, 4), np.uint8)
    want[:, :] = (114, 7, 250, 255)
    win = np.asarray(im.crop((sx, sy, sx + sw, sy + sh)).resize((dw, dh), _pil_filter(Image, kind)))
    want[dy:dy + dh, dx:dx + dw, :3] = win
    assert (ref.rgba(full, ow, oh, fc.rects(name), kind, (114, 7, 250)) == want).all()
    if (sw, sh) != size and dw > 1 and sw > 4:
        # ... which is not resize(box=...): that one reads pixels outside the window
        boxed = np.asarray(im.resize((dw, dh), _pil_filter(Image, kind), box=(sx, sy, sx + sw, sy + sh)))
        assert (boxed != win).any()


@pytest.mark.parametrize("kind", fc.KINDS, ids=fc.KIND_IDS)
def test_restatement_is_pillow_at_odd_and_tiny_sizes(kind):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    for (w, h), (ow, oh) in (((170, 131), (101, 33)), ((30, 20), (70, 50)), ((1, 1), (5, 3)), ((288, 288), (224, 224)),
                             ((352, 288), (640, 480)), ((352, 288), (224, 183))):
        pic = (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
        got = ref.resize(pic, ow, oh, kind)
        assert (got == np.asarray(Image.fromarray(pic, "RGB").resize((ow, oh), _pil_filter(Image, kind)))).all(), (w, h, ow, oh)
