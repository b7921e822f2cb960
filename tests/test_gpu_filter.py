"""GPU tests of the bilinear and bicubic resampling of a resized output (h263mi_filter: k_rgba_filter, k_tensor_filter).  Every
comparison is exact, against the oracle's planes -> full-size RGBA (test_gpu_rgba_layout.full_rgba) -> filter_ref (Pillow's
two-pass resampling of the source window, restated; pasted into the pad colour; tensor_out_ref.planes).  QCIF and CIF only: the
shapes are the ones the kernels are run at lane by lane on the CPU (filter_cases.CASES), where every hazard of theirs is shown to
occur; tests/test_filter.py shows that these pictures reach the clamp in both passes."""
import numpy as np
import pytest
import torch  # before the library is loaded: torch brings its own HIP runtime, which the C-ABI library must share (as in bench.py)

import filter_cases as fc
import filter_ref as flt
import framing_ref as fref
import h263mi
import recgen
import tensor_out_ref as ref
from oracle import oracle as orc
from test_gpu_rgba_layout import _small_streams, _upload_records, full_rgba

pytestmark = pytest.mark.gpu
SENTINEL = 0xC3
PAD = (114, 7, 250)
DTYPES = [ref.F32, ref.F16, ref.BF16]
IDS = ["f32", "f16", "bf16"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if h263mi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")


def _sentinel(dtype):
    return np.array([SENTINEL] * 4, np.uint8).view(ref.BITS_DTYPE[dtype])[0]


def _canvas(nbytes):
    c = h263mi.DeviceBuffer(nbytes)
    c.upload(np.full(nbytes, SENTINEL, np.uint8))
    return c


def _same(got, want, what):
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d elements differ, first at %s: %#x, want %#x" % (what, bad.size, bad[:8], got[bad[0]], want[bad[0]])


def _full(planes, w, h, strength):
    return full_rgba(planes, w, strength).reshape(h, w, 4)


def _framing(name, keep=False, pad=PAD):
    """the case's framing; a STRETCH case with nothing to say is no framing at all"""
    _, _, mode, s, d = fc.CASES[name]
    if mode == fref.STRETCH and not keep:
        return None
    return h263mi.make_framing(mode, pad=pad, keep_outside=keep, src=s if mode == fref.WINDOW else None,
                               dst=d if mode == fref.WINDOW else None)


# ---------------------------------------------------------------------------------------------
# 1. one state: every case x {bilinear, bicubic}, RGBA and the three dtypes, pad and keep_outside
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def states():
    """a QCIF and a CIF state with one I picture each, their full-size RGBA at strength 7, and the W' x H' RGBA of every case and
    kind with the pad colour around it: computed once"""
    out, sts = {}, []
    for w, h in (fc.QCIF, fc.CIF):
        mbs, co = recgen.intra_picture(w, h, seed=w + 5)
        rc, planes = orc.decode_picture(w, h, mbs, co, None)
        assert rc == 0
        st = h263mi.H263State(h263mi.SORENSON_SPARK_BITSTREAM, device_id=0)
        st.submit_picture(w, h, mbs, co, h263mi.PICTURE_I, temporal_reference=0, pquant=8)
        sts.append(st)
        out[(w, h)] = (st, _full(planes, w, h, 7))
    want = {}
    for name, (size, (ow, oh), _, _, _) in fc.CASES.items():
        for kind in fc.KINDS:
            want[(name, kind)] = flt.rgba(out[size][1], ow, oh, fc.rects(name), kind, PAD)
    yield out, want
    for st in sts:
        st.close()


@pytest.mark.parametrize("keep", [False, True], ids=["pad", "keep"])
@pytest.mark.parametrize("kind", fc.KINDS, ids=fc.KIND_IDS)
@pytest.mark.parametrize("name", list(fc.CASES))
def test_state_rgba_filtered(states, name, kind, keep):
    by_size, wants = states
    size, (ow, oh), _, _, _ = fc.CASES[name]
    st, _ = by_size[size]
    pitch = 4 * ow + 8
    nbytes = h263mi.rgba_resize_extent(1, ow, oh, pitch)
    out = np.full(nbytes + 4, SENTINEL, np.uint8)
    st.render_rgba_resize_filtered_into(7, out, _framing(name, keep), h263mi.make_filter(kind), ow, oh, pitch)
    want = np.full(nbytes + 4, SENTINEL, np.uint8)
    mask = fref.inside(fc.rects(name), oh, ow)
    for y in range(oh):
        row = want[y * pitch:y * pitch + 4 * ow].reshape(ow, 4)
        sel = mask[y] if keep else np.ones(ow, bool)
        row[sel] = wants[(name, kind)][y][sel]
    _same(out, want, name)


@pytest.mark.parametrize("keep", [False, True], ids=["pad", "keep"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", fc.KINDS, ids=fc.KIND_IDS)
@pytest.mark.parametrize("name", list(fc.CASES))
def test_state_tensor_filtered(states, name, kind, dtype, keep):
    by_size, wants = states
    size, (ow, oh), _, _, _ = fc.CASES[name]
    st, _ = by_size[size]
    bgr = dtype == ref.F16
    scale, bias = ref.EDGES if dtype == ref.F16 else ref.IMAGENET
    stride_h = ow + 3
    stride_c = oh * stride_h + 5
    t = h263mi.make_tensor_out(ow, oh, dtype, scale, bias, bgr=bgr, stride_h=stride_h, stride_c=stride_c)
    n_elem = 1 + h263mi.tensor_extent(1, t) // ref.ELT[dtype] + 7
    out = np.full(n_elem, _sentinel(dtype), ref.BITS_DTYPE[dtype])
    st.render_tensor_filtered_into(7, t, _framing(name, keep), h263mi.make_filter(kind), out[1:])
    want = np.full(n_elem, _sentinel(dtype), ref.BITS_DTYPE[dtype])
    pl = ref.planes(wants[(name, kind)], dtype, scale, bias, bgr)
    mask = fref.inside(fc.rects(name), oh, ow)
    for p in range(3):
        for y in range(oh):
            at = 1 + p * stride_c + y * stride_h
            sel = mask[y] if keep else np.ones(ow, bool)
            want[at:at + ow][sel] = pl[p, y][sel]
    _same(out, want, name)


def test_state_refusals_write_nothing(states):
    by_size, _ = states
    st, _ = by_size[fc.QCIF]
    ow, oh = 40, 30
    bad_kind = h263mi.make_filter(3)
    bad_reserved = h263mi.make_filter(flt.BICUBIC)
    bad_reserved.reserved[6] = 1
    t = h263mi.make_tensor_out(ow, oh, ref.F32)
    for bad in (bad_kind, bad_reserved):
        out = np.full(4 * ow * oh, SENTINEL, np.uint8)
        with pytest.raises(h263mi.H263Error) as e:
            st.render_rgba_resize_filtered_into(7, out, None, bad, ow, oh)
        assert e.value.code == h263mi.ERR_INVALID_ARGUMENT and (out == SENTINEL).all()
        out = np.full(3 * ow * oh, _sentinel(ref.F32), np.uint32)
        with pytest.raises(h263mi.H263Error) as e:
            st.render_tensor_filtered_into(7, t, None, bad, out)
        assert e.value.code == h263mi.ERR_INVALID_ARGUMENT and (out == _sentinel(ref.F32)).all()


# ---------------------------------------------------------------------------------------------
# 2. AREA through the new entry points is the _framed call, byte for byte
# ---------------------------------------------------------------------------------------------
def test_area_through_the_filtered_entry_points_is_the_framed_call(states):
    by_size, _ = states
    st, _ = by_size[fc.CIF]
    area = h263mi.make_filter(flt.AREA)
    for name in ("cif_50x37", "cif_letterbox_224", "cif_window_300"):
        _, (ow, oh), _, _, _ = fc.CASES[name]
        f = _framing(name)
        want = st.render_rgba_resize_framed(7, f, ow, oh)
        for fl in (None, area):
            _same(st.render_rgba_resize_filtered(7, f, fl, ow, oh), want, name)
        t = h263mi.make_tensor_out(ow, oh, ref.BF16, *ref.IMAGENET)
        want_t = np.zeros(3 * oh * ow, np.uint16)
        st.render_tensor_framed_into(7, t, f, want_t)
        for fl in (None, area):
            got = np.zeros(3 * oh * ow, np.uint16)
            st.render_tensor_filtered_into(7, t, f, fl, got)
            _same(got, want_t, name + " tensor")
    # a batch: the fused half-size layout stays the fused layout
    n, w, h = 2, 352, 288
    recs, planes = _upload_records(_small_streams(n, w, h, 8600), w, h)
    outs = []
    for filtered in (False, True):
        b = h263mi.Batch(n, w, h, 0, None)
        if filtered:
            b.set_rgba_resize_filtered(h263mi.make_framing(fref.LETTERBOX, pad=PAD), area, 176, 144)
        else:
            b.set_rgba_resize_framed(h263mi.make_framing(fref.LETTERBOX, pad=PAD), 176, 144)
        c = _canvas(h263mi.rgba_resize_extent(n, 176, 144))
        b.decode(h263mi.PICTURE_I, recs[0].ptr, recs[1].ptr, recs[2].ptr, 0, 5, c.ptr, None)
        b.sync()
        outs.append(c.download())
        b.close()
    _same(outs[1], outs[0], "filtered AREA against framed")


# ---------------------------------------------------------------------------------------------
# 3. a batch of 3 QCIF streams, one inactive: immediate, and pipelined with the shape changed between request and delivery
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def qcif3():
    n, w, h = 3, 176, 144
    recs = [_upload_records(_small_streams(n, w, h, 8100 + 100 * k), w, h) for k in range(3)]
    return n, w, h, recs


def _tensor_canvas(n_elem, dtype, pics, t, base, stride_n, skip=()):
    want = np.full(n_elem, _sentinel(dtype), ref.BITS_DTYPE[dtype])
    for s, pic in enumerate(pics):
        if s not in skip:
            ref.place(want, ref.planes(pic, dtype, list(t.scale), list(t.bias), bool(t.bgr)), base + s * stride_n, t.stride_c, t.stride_h)
    return want


def _filtered_pics(planes, w, h, strength, ow, oh, rects, kind, pad):
    return [flt.rgba(_full(p, w, h, strength), ow, oh, rects, kind, pad) for p in planes]


@pytest.mark.parametrize("kind", fc.KINDS, ids=fc.KIND_IDS)
def test_batch_immediate_one_stream_inactive(qcif3, kind):
    n, w, h, recs = qcif3
    ow, oh = 96, 96
    grey = (114, 114, 114)
    f = h263mi.make_framing(fref.LETTERBOX, pad=grey)
    rects = fref.resolve(w, h, ow, oh, fref.LETTERBOX)
    dtype = ref.BF16
    stride_h = ow + 3
    stride_c = oh * stride_h + 5
    stride_n = 3 * stride_c + 7
    t = h263mi.make_tensor_out(ow, oh, dtype, *ref.IMAGENET, bgr=True, stride_n=stride_n, stride_c=stride_c, stride_h=stride_h)
    nbytes = h263mi.tensor_extent(n, t)
    n_elem = 1 + nbytes // 2 + 5
    b = h263mi.Batch(n, w, h, 0, None)
    b.set_tensor_output_filtered(t, f, h263mi.make_filter(kind))
    b.set_active([1, 0, 1])
    c = _canvas(n_elem * 2)
    (mbs, co, base), planes = recs[0]
    b.decode(h263mi.PICTURE_I, mbs.ptr, co.ptr, base.ptr, 0, 5, c.at(2), None)
    b.sync()
    want = _tensor_canvas(n_elem, dtype, _filtered_pics(planes, w, h, 5, ow, oh, rects, kind, grey), t, 1, stride_n, skip=(1,))
    _same(c.download().view(np.uint16), want, "tensor")
    # the same batch as RGBA without a framing: the filter replaces the tensor
    b.set_rgba_resize_filtered(None, h263mi.make_filter(kind), 224, 224)
    c2 = _canvas(h263mi.rgba_resize_extent(n, 224, 224))
    b.render_rgba(5, c2.ptr, None)
    b.sync()
    whole = ((0, 0, w, h), (0, 0, 224, 224))
    want2 = np.full((n, 224, 224, 4), SENTINEL, np.uint8)
    for s in (0, 2):
        want2[s] = flt.rgba(_full(planes[s], w, h, 5), 224, 224, whole, kind)
    _same(c2.download(), want2, "rgba")
    b.close()


def test_pipelined_output_keeps_the_filter_of_its_request(qcif3):
    n, w, h, recs = qcif3
    b = h263mi.Batch(n, w, h, 0, None, pipeline_post=True)
    b.set_active([1, 0, 1])
    # call 1: RGBA bicubic 224 x 224; call 2: bf16 tensor, bilinear, cover 50 x 70; call 3: the area average 40 x 30
    tb = h263mi.make_tensor_out(50, 70, ref.BF16, *ref.IMAGENET)
    fb = h263mi.make_framing(fref.COVER, pad=PAD)
    c1 = _canvas(h263mi.rgba_resize_extent(n, 224, 224))
    c2 = _canvas(h263mi.tensor_extent(n, tb))
    c3 = _canvas(h263mi.rgba_resize_extent(n, 40, 30))
    dec = lambda k, strength, c: b.decode(h263mi.PICTURE_I, recs[k][0][0].ptr, recs[k][0][1].ptr, recs[k][0][2].ptr, 0, strength, c.ptr, None)
    cubic = h263mi.make_filter(flt.BICUBIC)
    b.set_rgba_resize_filtered(None, cubic, 224, 224)
    dec(0, 7, c1)                                                     # deferred
    cubic.kind = flt.BILINEAR                                         # (the filter was copied)
    b.set_tensor_output_filtered(tb, fb, h263mi.make_filter(flt.BILINEAR))
    dec(1, 3, c2)                                                     # renders 1 -- under the shape of ITS request
    b.set_rgba_resize(40, 30)
    dec(2, 9, c3)                                                     # renders 2
    b.set_rgba_resize_filtered(None, h263mi.make_filter(flt.BICUBIC), 224, 224)
    b.sync()                                                          # renders 3
    whole = ((0, 0, w, h), (0, 0, 224, 224))
    want1 = np.full((n, 224, 224, 4), SENTINEL, np.uint8)
    for s in (0, 2):
        want1[s] = flt.rgba(_full(recs[0][1][s], w, h, 7), 224, 224, whole, flt.BICUBIC)
    _same(c1.download(), want1, "call 1")
    pics2 = _filtered_pics(recs[1][1], w, h, 3, 50, 70, fref.resolve(w, h, 50, 70, fref.COVER), flt.BILINEAR, PAD)
    _same(c2.download().view(np.uint16), _tensor_canvas(c2.nbytes // 2, ref.BF16, pics2, tb, 0, 3 * 70 * 50, skip=(1,)), "call 2")
    import rgba_resize_ref
    want3 = np.full((n, 30, 40, 4), SENTINEL, np.uint8)
    for s in (0, 2):
        want3[s] = rgba_resize_ref.resize(full_rgba(recs[2][1][s], w, 9), w, h, 40, 30).reshape(30, 40, 4)
    _same(c3.download(), want3, "call 3")
    b.close()


def test_batch_refusals_keep_the_shape(qcif3):
    n, w, h, recs = qcif3
    b = h263mi.Batch(n, w, h, 0, None)
    good = h263mi.make_filter(flt.BILINEAR)
    b.set_rgba_resize_filtered(None, good, 65, 5)
    bad_kind, bad_reserved = h263mi.make_filter(3), h263mi.make_filter(flt.BILINEAR)
    bad_reserved.reserved[0] = 1
    t = h263mi.make_tensor_out(65, 5, ref.F32)
    for bad in (bad_kind, bad_reserved):
        with pytest.raises(h263mi.H263Error) as e:
            b.set_rgba_resize_filtered(None, bad, 9, 9)
        assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
        with pytest.raises(h263mi.H263Error) as e:
            b.set_tensor_output_filtered(t, None, bad)
        assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    with pytest.raises(h263mi.H263Error) as e:                        # a refused framing under a good filter
        b.set_rgba_resize_filtered(h263mi.make_framing(fref.WINDOW, src=(0, 0, w + 1, h), dst=(0, 0, 9, 9)), good, 9, 9)
    assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    c = _canvas(h263mi.rgba_resize_extent(n, 65, 5))
    (mbs, co, base), planes = recs[0]
    b.decode(h263mi.PICTURE_I, mbs.ptr, co.ptr, base.ptr, 0, 5, c.ptr, None)
    b.sync()
    whole = ((0, 0, w, h), (0, 0, 65, 5))
    want = np.stack([flt.rgba(_full(p, w, h, 5), 65, 5, whole, flt.BILINEAR) for p in planes])
    _same(c.download(), want, "after the refusals")
    b.close()


# ---------------------------------------------------------------------------------------------
# 4. a mixed-size set: QCIF and CIF into one [n, 3, 224, 224] bf16 tensor, every size its own rectangle and its own taps
# ---------------------------------------------------------------------------------------------
class _Part:
    """a part of a device buffer, as MixedBatch.decode_next_pictures takes it"""

    def __init__(self, buf, offset, nbytes):
        self.ptr, self.nbytes = buf.at(offset), nbytes


@pytest.mark.parametrize("kind", fc.KINDS, ids=fc.KIND_IDS)
def test_mixed_set_letterboxed_into_one_bf16_tensor(kind):
    import sorenson_enc as enc
    from test_bitstream_e2e import make_codable
    q, strength = 6, 5
    sizes = [(176, 144), (352, 288), (176, 144), (320, 240)]
    n, ow, oh, dtype = len(sizes), 224, 224, ref.BF16
    grey = (114, 114, 114)
    f = h263mi.make_framing(fref.LETTERBOX, pad=grey)
    fl = h263mi.make_filter(kind)
    t = h263mi.make_tensor_out(ow, oh, dtype, *ref.IMAGENET)
    one = h263mi.tensor_extent(1, t)
    m = h263mi.MixedBatch(n)
    with pytest.raises(h263mi.H263Error) as e:                        # WINDOW stays refused
        m.set_tensor_output_filtered(t, h263mi.make_framing(fref.WINDOW, src=(0, 0, 8, 8), dst=(0, 0, 8, 8)), fl)
    assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    with pytest.raises(h263mi.H263Error) as e:
        m.set_rgba_resize_filtered(f, h263mi.make_filter(7), ow, oh)
    assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    m.set_tensor_output_filtered(t, f, fl)
    buf = _canvas(n * one)
    datas, wants, rects = [], [], []
    for s, (w, h) in enumerate(sizes):
        mbs, co = recgen.intra_picture(w, h, seed=8700 + s, max_level=60)
        mbs = make_codable(mbs, q, s, 0)
        datas.append(enc.encode_picture(w, h, 0, q, mbs, co, temporal_reference=0))
        rc, planes = orc.decode_picture(w, h, mbs, co, None)
        assert rc == 0
        rects.append(fref.resolve(w, h, ow, oh, fref.LETTERBOX))
        wants.append(flt.rgba(_full(planes, w, h, strength), ow, oh, rects[-1], kind, grey))
    parts = [_Part(buf, s * one, one) for s in range(n)]
    used, rcs, _ = m.decode_next_pictures(datas, n_threads=2, strength=strength, rgba=parts)
    assert not any(m.sync()) and list(rcs) == [0] * n
    for s in range(n):
        got = m.stream_framing(s)
        assert (got.src(), got.dst()) == rects[s]
    assert rects[0][1] == rects[1][1] == (0, 20, 224, 183) and rects[3][1] == (0, 28, 224, 168)
    _same(buf.download().view(np.uint16), _tensor_canvas(n * one // 2, dtype, wants, t, 0, 3 * oh * ow), "the tensor")
    # what is really allocated counts: the full-size pictures of every class (slots: a power of two) and its own tap tables
    with_filter = m.frame_store_bytes()
    m.set_tensor_output(None)
    bare = m.frame_store_bytes()
    tables = 0
    for (w, h), slots in (((176, 144), 2), ((352, 288), 1), ((320, 240), 1)):
        (_, _, sw, sh), (_, _, dw, dh) = fref.resolve(w, h, ow, oh, fref.LETTERBOX)
        tables += 4 * w * h * slots + 8 * (dw + dh) + 4 * (dw * flt.taps(kind, sw, dw)[0] + dh * flt.taps(kind, sh, dh)[0])
    assert with_filter - bare == tables
    m.close()
