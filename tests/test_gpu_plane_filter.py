"""GPU tests of the bilinear and bicubic resampling of the resized YUV output (h263mi_batch_set_yuv_resize_filtered,
h263mi_render_yuv_resize_filtered: k_plane_filter).  Every comparison is exact, against the oracle's planes, deblocked, put
through plane_filter_ref (Pillow's two-pass resampling per plane, restated; tests/test_plane_filter.py holds it to Pillow) and
placed by yuv_layout_ref into a sentinel canvas.  QCIF, CIF and 75 x 51 only: the shapes are the ones the kernel is run at lane by
lane on the CPU (plane_filter_cases.GPU_CASES), where every hazard of theirs is shown to occur."""
import numpy as np
import pytest
import torch  # before the library is loaded: torch brings its own HIP runtime, which the C-ABI library must share (as in bench.py)

import filter_ref as flt
import h263mi
import plane_filter_cases as pc
import plane_filter_ref as ref
import tensor_out_ref as tref
import yuv_layout_ref as lay
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
SENTINEL = 0xC3
S = pc.STRENGTH
FORMATS = [h263mi.YUV_I420, h263mi.YUV_NV12]
PLACEMENTS = ["tight", "odd", "shifted"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if h263mi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")


def _canvas(nbytes):
    c = h263mi.DeviceBuffer(nbytes)
    c.upload(np.full(nbytes, SENTINEL, np.uint8))
    return c


def _same(got, want, what):
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d elements differ, first at %s: %#x, want %#x" % (what, bad.size, bad[:8], got[bad[0]], want[bad[0]])


def _placed(nbytes, base, pics, ow, oh, fmt, py, pcc, offs, skip=()):
    want = np.full(nbytes, SENTINEL, np.uint8)
    ref.place(want[base:], pics, ow, oh, fmt, py, pcc, *offs, skip=skip)
    return want


def _resize(ow, oh, fmt, py, pcc, offs, given):
    """-> (YuvResize, what keeps its offset arrays alive)"""
    return h263mi.make_yuv_resize(ow, oh, fmt, py, pcc, *(offs if given else (None, None, None)))


# ---------------------------------------------------------------------------------------------
# 1. one state: every case x {bilinear, bicubic} x {I420, NV12} x the three placements
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def states():
    out = {}
    for size in pc.SIZES:
        w, h = size
        mbs, co = pc.records(size, 0)
        st = h263mi.H263State(h263mi.SORENSON_SPARK_BITSTREAM, device_id=0)
        st.submit_picture(w, h, mbs, co, h263mi.PICTURE_I, temporal_reference=0, pquant=8)
        out[size] = st
    yield out
    for st in out.values():
        st.close()


@pytest.mark.parametrize("kind", pc.KINDS, ids=pc.KIND_IDS)
@pytest.mark.parametrize("name", pc.GPU_CASES)
def test_state_yuv_resize_filtered(states, name, kind):
    size, (ow, oh) = pc.CASES[name]
    st = states[size]
    pics = [pc.want(name, kind, 0)]
    f = h263mi.make_filter(kind)
    for fmt in FORMATS:
        for placement in PLACEMENTS:
            py, pcc, offs, given, base, nbytes = ref.placements(ow, oh, fmt, 1)[placement]
            out = np.full(nbytes, SENTINEL, np.uint8)
            r, keep = _resize(ow, oh, fmt, py, pcc, offs, given)
            st.render_yuv_resize_filtered_into(S, out[base:], f, 0, 0, resize=r)
            _same(out, _placed(nbytes, base, pics, ow, oh, fmt, py, pcc, offs), "%s format %d %s" % (name, fmt, placement))
            del keep


def test_state_area_null_identity_and_refusals(states):
    st = states[pc.QCIF]
    w, h = pc.QCIF
    area, cubic = h263mi.make_filter(flt.AREA), h263mi.make_filter(flt.BICUBIC)
    for fmt in FORMATS:
        want = st.render_yuv_resize(S, 100, 37, fmt)
        for f in (None, area):
            _same(st.render_yuv_resize_filtered(S, f, 100, 37, fmt), want, "AREA / NULL is the unfiltered call")
        # W' = w, H' = h under any filter is the full-size layout, byte for byte
        _same(st.render_yuv_resize_filtered(S, cubic, w, h, fmt, 256, 256), st.render_yuv(S, fmt, 256, 256), "identity")
    bad_kind, bad_reserved = h263mi.make_filter(3), h263mi.make_filter(flt.BILINEAR)
    bad_reserved.reserved[2] = 1
    for bad in (bad_kind, bad_reserved):
        out = np.full(40 * 30 * 2, SENTINEL, np.uint8)
        with pytest.raises(h263mi.H263Error) as e:
            st.render_yuv_resize_filtered_into(S, out, bad, 40, 30)
        assert e.value.code == h263mi.ERR_INVALID_ARGUMENT and (out == SENTINEL).all()
    # the strength the picture's own header asks for (USE_DEBLOCKER is not set here: none)
    _same(st.render_yuv_resize_filtered(h263mi.STRENGTH_FROM_HEADER, cubic, 40, 30), st.render_yuv_resize_filtered(0, cubic, 40, 30), "header")


# ---------------------------------------------------------------------------------------------
# 2. a batch of 3 QCIF streams with distinct pictures, stream 1 without a picture; per-stream offset arrays
# ---------------------------------------------------------------------------------------------
N = 3
SKIP = (1,)


def _upload(pics):
    mbs = np.concatenate([m for m, _ in pics])
    co = np.concatenate([c for _, c in pics]).astype(np.int16)
    base = np.cumsum([0] + [c.shape[0] for _, c in pics[:-1]]).astype(np.uint64)
    bufs = []
    for arr in (mbs, co, base):
        d = h263mi.DeviceBuffer(max(arr.nbytes, 16))
        d.upload(arr)
        bufs.append(d)
    return bufs


@pytest.fixture(scope="module")
def qcif3():
    return _upload([pc.records(pc.QCIF, s) for s in range(N)])


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("fmt", FORMATS, ids=["i420", "nv12"])
@pytest.mark.parametrize("kind", pc.KINDS, ids=pc.KIND_IDS)
def test_batch_immediate_one_stream_without_a_picture(qcif3, kind, fmt, placement):
    name = "qcif_224"
    _, (ow, oh) = pc.CASES[name]
    py, pcc, offs, given, base, nbytes = ref.placements(ow, oh, fmt, N)[placement]
    b = h263mi.Batch(N, 176, 144, 0, None)
    r, keep = _resize(ow, oh, fmt, py, pcc, offs, given)
    b.set_yuv_resize_filtered(r, h263mi.make_filter(kind))
    del keep                                                          # (the offsets were copied)
    b.set_active([1, 0, 1])
    c = _canvas(nbytes)
    b.decode(h263mi.PICTURE_I, qcif3[0].ptr, qcif3[1].ptr, qcif3[2].ptr, 0, S, None, c.at(base))
    b.sync()
    pics = [pc.want(name, kind, s) for s in range(N)]
    _same(c.download(), _placed(nbytes, base, pics, ow, oh, fmt, py, pcc, offs, skip=SKIP), "decode")
    # every stream's last picture, rendered again: stream 1 has none
    c2 = _canvas(nbytes)
    b.render_rgba(S, None, c2.at(base))
    b.sync()
    _same(c2.download(), _placed(nbytes, base, pics, ow, oh, fmt, py, pcc, offs, skip=SKIP), "render")
    b.close()


def test_filtered_planes_and_a_filtered_tensor_in_one_call(qcif3):
    from test_gpu_rgba_layout import full_rgba
    name, kind, fmt = "qcif_224", flt.BICUBIC, h263mi.YUV_NV12
    w, h = pc.QCIF
    _, (ow, oh) = pc.CASES[name]
    py, pcc, offs, given, base, nbytes = ref.placements(ow, oh, fmt, N)["shifted"]
    tw, th, dtype = 96, 80, tref.BF16
    t = h263mi.make_tensor_out(tw, th, dtype, *tref.IMAGENET)
    b = h263mi.Batch(N, w, h, 0, None)
    r, keep = _resize(ow, oh, fmt, py, pcc, offs, given)
    b.set_yuv_resize_filtered(r, h263mi.make_filter(kind))
    b.set_tensor_output_filtered(t, None, h263mi.make_filter(flt.BILINEAR))
    b.set_active([1, 0, 1])
    cy, ct = _canvas(nbytes), _canvas(h263mi.tensor_extent(N, t))
    b.decode(h263mi.PICTURE_I, qcif3[0].ptr, qcif3[1].ptr, qcif3[2].ptr, 0, S, ct.ptr, cy.at(base))
    b.sync()
    _same(cy.download(), _placed(nbytes, base, [pc.want(name, kind, s) for s in range(N)], ow, oh, fmt, py, pcc, offs, skip=SKIP), "planes")
    want = np.full(ct.nbytes // 2, np.array([SENTINEL] * 2, np.uint8).view(np.uint16)[0], np.uint16)
    whole = ((0, 0, w, h), (0, 0, tw, th))
    for s in range(N):
        if s in SKIP:
            continue
        rc, planes = orc.decode_picture(w, h, *pc.records(pc.QCIF, s), None)
        assert rc == 0
        rgba = flt.rgba(full_rgba(planes, w, S).reshape(h, w, 4), tw, th, whole, flt.BILINEAR)
        tref.place(want, tref.planes(rgba, dtype, *tref.IMAGENET, False), s * 3 * th * tw)
    _same(ct.download().view(np.uint16), want, "tensor")
    b.close()


def test_pipelined_planes_keep_the_filter_of_their_request(qcif3):
    """the filter is set, a picture decoded, the shape changed to the area average before the deferred rendering is delivered: the
    output is the filtered one"""
    import yuv_resize_ref
    name, kind, fmt = "qcif_257x5", flt.BICUBIC, h263mi.YUV_I420
    w, h = pc.QCIF
    _, (ow, oh) = pc.CASES[name]
    py, pcc, offs, given, base, nbytes = ref.placements(ow, oh, fmt, N)["odd"]
    b = h263mi.Batch(N, w, h, 0, None, pipeline_post=True)
    b.set_active([1, 0, 1])
    r, keep = _resize(ow, oh, fmt, py, pcc, offs, given)
    cubic = h263mi.make_filter(kind)
    b.set_yuv_resize_filtered(r, cubic)
    c1 = _canvas(nbytes)
    b.decode(h263mi.PICTURE_I, qcif3[0].ptr, qcif3[1].ptr, qcif3[2].ptr, 0, S, None, c1.at(base))     # deferred
    cubic.kind = flt.BILINEAR                                                                      # (the filter was copied)
    b.set_yuv_resize_filtered(r, h263mi.make_filter(flt.AREA))
    c2 = _canvas(nbytes)
    b.decode(h263mi.PICTURE_I, qcif3[0].ptr, qcif3[1].ptr, qcif3[2].ptr, 0, S, None, c2.at(base))     # k_frame renders call 1
    b.set_yuv_resize_filtered(None, None)
    b.sync()                                                                                       # ... and k_post call 2
    _same(c1.download(), _placed(nbytes, base, [pc.want(name, kind, s) for s in range(N)], ow, oh, fmt, py, pcc, offs, skip=SKIP), "call 1")
    area = [yuv_resize_ref.resize_planes(pc.picture(pc.QCIF, s), w, h, ow, oh) for s in range(N)]
    _same(c2.download(), _placed(nbytes, base, area, ow, oh, fmt, py, pcc, offs, skip=SKIP), "call 2")
    b.close()


def test_batch_area_null_identity_and_refusals(qcif3):
    w, h = pc.QCIF
    ow, oh, fmt, py, pcc = 100, 37, h263mi.YUV_NV12, 128, 128
    nbytes = h263mi.yuv_resize_extent(N, ow, oh, fmt, py, pcc)

    def rendered(b, nb=nbytes):
        c = _canvas(nb)
        b.render_rgba(S, None, c.ptr)
        b.sync()
        return c.download()
    b = h263mi.Batch(N, w, h, 0, None)
    b.decode(h263mi.PICTURE_I, qcif3[0].ptr, qcif3[1].ptr, qcif3[2].ptr, 0, S, None, None)
    b.sync()
    b.set_yuv_resize(ow, oh, fmt, py, pcc)
    want = rendered(b)
    r, keep = h263mi.make_yuv_resize(ow, oh, fmt, py, pcc)
    for f in (None, h263mi.make_filter(flt.AREA)):
        b.set_yuv_resize_filtered(None, None)
        b.set_yuv_resize_filtered(r, f)
        _same(rendered(b), want, "AREA / NULL is set_yuv_resize")
    # a refused filter leaves the shape in force untouched
    cubic = h263mi.make_filter(flt.BICUBIC)
    b.set_yuv_resize_filtered(r, cubic)
    filtered = rendered(b)
    pics = [ref.planes(*pc.picture(pc.QCIF, s), ow, oh, flt.BICUBIC, w, h) for s in range(N)]
    _same(filtered, _placed(nbytes, 0, pics, ow, oh, fmt, py, pcc, lay.default_offsets(N, ow, oh, fmt, py, pcc)), "bicubic")
    bad_kind, bad_reserved = h263mi.make_filter(3), h263mi.make_filter(flt.BICUBIC)
    bad_reserved.reserved[0] = 1
    other, keep2 = h263mi.make_yuv_resize(9, 9)
    for bad in (bad_kind, bad_reserved):
        with pytest.raises(h263mi.H263Error) as e:
            b.set_yuv_resize_filtered(other, bad)
        assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    _same(rendered(b), filtered, "after the refusals")
    # a checked batch holds d_deblocked to the extent under a filter too
    small = h263mi.DeviceBuffer(nbytes - 1)
    with pytest.raises(h263mi.H263Error) as e:
        b.render_rgba(S, None, small.ptr)
    assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    # W' = w, H' = h under a filter is the full-size layout; a layout replaces the filtered resize and is replaced by it
    full, keep3 = h263mi.make_yuv_resize(w, h, h263mi.YUV_I420, 256, 128)
    nb = h263mi.yuv_layout_extent(N, w, h, h263mi.YUV_I420, 256, 128)
    b.set_yuv_resize_filtered(full, cubic)
    identity = rendered(b, nb)
    b.set_yuv_layout(h263mi.YUV_I420, 256, 128)
    _same(identity, rendered(b, nb), "identity is the layout")
    b.set_yuv_resize_filtered(r, cubic)
    _same(rendered(b), filtered, "filtered after a layout")
    b.close()


# ---------------------------------------------------------------------------------------------
# 3. H263MI_STRENGTH_FROM_HEADER through h263mi_batch_decode_next_pictures_ps under a filtered YUV shape
# ---------------------------------------------------------------------------------------------
def test_strength_from_header_under_a_filtered_yuv_shape():
    from test_gpu_round6 import _Streams, header_strength
    n, w, h = 4, 176, 144
    ow, oh, fmt, kind = 50, 37, h263mi.YUV_NV12, flt.BICUBIC
    st = _Streams(n, w, h, seed=2101)
    b = h263mi.Batch(n, w, h)
    r, keep = h263mi.make_yuv_resize(ow, oh, fmt)
    b.set_yuv_resize_filtered(r, h263mi.make_filter(kind))
    nbytes = h263mi.yuv_resize_extent(n, ow, oh, fmt)
    cw = (w + 1) // 2
    strengths = set()
    for f in range(2):
        datas = st.pictures(intra=f == 0)
        c = _canvas(nbytes)
        used, rcs = b.decode_next_pictures_ex(datas, n_threads=2, strength=h263mi.STRENGTH_FROM_HEADER, d_deblocked=c.ptr)
        assert not any(rcs), rcs
        b.sync()
        pics = []
        for s in range(n):
            k = header_strength(st.q[s], st.flag[s])
            strengths.add(k)
            planes = st.refs[s] if k == 0 else tuple(orc.deblock(p, pw, k) for p, pw in zip(st.refs[s], (w, cw, cw)))
            pics.append(ref.planes(*planes, ow, oh, kind, w, h))
        _same(c.download(), _placed(nbytes, 0, pics, ow, oh, fmt, ow, 2 * ((ow + 1) // 2), lay.default_offsets(n, ow, oh, fmt)), "frame %d" % f)
    assert len(strengths) >= 2
    b.close()
