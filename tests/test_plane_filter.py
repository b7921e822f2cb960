"""Bilinear and bicubic resampling of the resized YUV output (h263mi_batch_set_yuv_resize_filtered,
h263mi_render_yuv_resize_filtered): what needs no device.  The restatement (plane_filter_ref.planes) against Pillow, whose
Image.resize on a mode-L image is the definition, for every case of plane_filter_cases and both kinds; the extents, which the
filter does not change; the refusals that are decided before any device call; the two exports in the header and in the binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import filter_ref as flt
import h263mi
import plane_filter_cases as pc
import plane_filter_ref as ref
import yuv_layout_ref as lay
import yuv_resize_ref

BAD = h263mi.ERR_INVALID_ARGUMENT
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("h263mi_batch_set_yuv_resize_filtered", "h263mi_render_yuv_resize_filtered")


def _pil_filter(Image, kind):
    resampling = getattr(Image, "Resampling", Image)
    return resampling.BILINEAR if kind == flt.BILINEAR else resampling.BICUBIC


@pytest.mark.parametrize("kind", pc.KINDS, ids=pc.KIND_IDS)
@pytest.mark.parametrize("name", list(pc.CASES))
def test_restatement_is_pillow_mode_l_per_plane(name, kind):
    Image = pytest.importorskip("PIL.Image")
    (w, h), (ow, oh) = pc.CASES[name]
    (cw, ch), (cow, coh) = lay.chroma_size(w, h), lay.chroma_size(ow, oh)
    for index in (0, 2):
        pic = pc.picture((w, h), index)
        got = pc.want(name, kind, index)
        for g, p, (pw, ph), (pow_, poh) in zip(got, pic, ((w, h), (cw, ch), (cw, ch)), ((ow, oh), (cow, coh), (cow, coh))):
            im = Image.fromarray(np.ascontiguousarray(p.reshape(ph, pw)), "L")
            want = np.asarray(im.resize((pow_, poh), _pil_filter(Image, kind)))
            assert g.shape == (pow_ * poh,) and (g.reshape(poh, pow_) == want).all(), (name, kind, index)


def test_full_size_is_the_planes_themselves():
    pic = pc.picture(pc.QCIF)
    for kind in pc.KINDS:
        for g, p in zip(pc.want("identity", kind), pic):
            assert (g == p).all()


def test_the_extent_does_not_depend_on_the_filter():
    """h263mi_yuv_resize_extent is the one entry point for both forms: its values are the restatement's, at every placement the
    kernel is checked at"""
    for name in pc.CASES:
        _, (ow, oh) = pc.CASES[name]
        for fmt in (h263mi.YUV_I420, h263mi.YUV_NV12):
            for placement, (py, pcc, offs, given, base, nbytes) in ref.placements(ow, oh, fmt, 3).items():
                args = offs if given else (None, None, None)
                want = yuv_resize_ref.extent(3, ow, oh, fmt, py, pcc, *args)
                assert want is not None and want + base <= nbytes
                assert h263mi.yuv_resize_extent(3, ow, oh, fmt, py, pcc, *args) == want, (name, fmt, placement)
    assert h263mi.yuv_resize_extent(64, 640, 360, h263mi.YUV_NV12) == 64 * 640 * 360 * 3 // 2


def test_refusals_need_no_device():
    L = h263mi.lib()
    r, keep = h263mi.make_yuv_resize(40, 30)
    out = np.full(40 * 30 * 2, 0xC3, np.uint8)
    p = out.ctypes.data_as(C.c_void_p)
    good, bad_kind, bad_reserved = h263mi.make_filter(flt.BICUBIC), h263mi.make_filter(3), h263mi.make_filter(flt.BILINEAR)
    bad_reserved.reserved[6] = 1
    for f in (None, good, bad_kind, bad_reserved):
        fp = C.byref(f) if f is not None else None
        assert L.h263mi_batch_set_yuv_resize_filtered(None, C.byref(r), fp) == BAD         # no batch
        assert L.h263mi_render_yuv_resize_filtered(None, 0, C.byref(r), fp, p) == BAD      # no state
    assert (out == 0xC3).all()
    del keep


def test_both_exports_are_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "h263mi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in h263mi.EXPORTS and hasattr(h263mi.lib(), name)
    assert len(h263mi.lib().h263mi_batch_set_yuv_resize_filtered.argtypes) == 3
    assert len(h263mi.lib().h263mi_render_yuv_resize_filtered.argtypes) == 5
    assert h263mi.lib().h263mi_abi_version() == 7
    # the sentence that said the planes stay area-only is gone; what stays unoffered is said
    assert "stays area-only" not in src
    for phrase in ("a framing of YUV output", "mixed-size sets", "Lanczos and Hamming"):
        assert phrase in src
