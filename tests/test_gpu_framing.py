"""GPU tests of the framing of a resized output (h263mi_framing: k_rgba_resize_framed, k_tensor_resize_framed).  Every comparison
is exact, against the oracle's planes -> full-size RGBA (test_gpu_rgba_layout.full_rgba) -> framing_ref (rgba_resize_ref.resize of
the source window pasted into the pad colour, tensor_out_ref.planes).  QCIF and CIF only: the shapes are the ones the kernels are
run at lane by lane on the CPU (framing_cases.CASES), where every hazard of theirs is shown to occur."""
import numpy as np
import pytest
import torch  # before the library is loaded: torch brings its own HIP runtime, which the C-ABI library must share (as in bench.py)

import framing_cases as fc
import framing_ref as fref
import h263mi
import recgen
import rgba_resize_ref
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
    _, _, mode, s, d = fc.CASES[name]
    return h263mi.make_framing(mode, pad=pad, keep_outside=keep, src=s if mode == fref.WINDOW else None,
                               dst=d if mode == fref.WINDOW else None)


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


# ---------------------------------------------------------------------------------------------
# 1. one state: the four modes, RGBA and the three dtypes, at the shapes of the CPU checker, pad and keep_outside
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def states():
    """a QCIF and a CIF state with one I picture each, their full-size RGBA at strength 7, and the framed W' x H' RGBA of every
    case with the pad colour around it: computed once"""
    out, sts = {}, []
    for w, h in (fc.QCIF, fc.CIF):
        mbs, co = recgen.intra_picture(w, h, seed=w + 5)
        rc, planes = orc.decode_picture(w, h, mbs, co, None)
        assert rc == 0
        st = h263mi.H263State(h263mi.SORENSON_SPARK_BITSTREAM, device_id=0)
        st.submit_picture(w, h, mbs, co, h263mi.PICTURE_I, temporal_reference=0, pquant=8)
        sts.append(st)
        out[(w, h)] = (st, _full(planes, w, h, 7))
    framed = {}
    for name, ((w, h), (ow, oh), _, _, _) in fc.CASES.items():
        framed[name] = fref.rgba(out[(w, h)][1], ow, oh, fc.rects(name), PAD)
    yield out, framed
    for st in sts:
        st.close()


@pytest.mark.parametrize("keep", [False, True], ids=["pad", "keep"])
@pytest.mark.parametrize("name", list(fc.CASES))
def test_state_rgba_framed(states, name, keep):
    by_size, framed = states
    (w, h), (ow, oh), _, _, _ = fc.CASES[name]
    st, _ = by_size[(w, h)]
    rc = fc.rects(name)
    pitch = 4 * ow + 8
    nbytes = h263mi.rgba_resize_extent(1, ow, oh, pitch)
    out = np.full(nbytes + 4, SENTINEL, np.uint8)
    st.render_rgba_resize_framed_into(7, out, _framing(name, keep), ow, oh, pitch)
    want = np.full(nbytes + 4, SENTINEL, np.uint8)
    mask = fref.inside(rc, oh, ow)
    for y in range(oh):
        row = want[y * pitch:y * pitch + 4 * ow].reshape(ow, 4)
        sel = mask[y] if keep else np.ones(ow, bool)
        row[sel] = framed[name][y][sel]
    _same(out, want, name)


@pytest.mark.parametrize("keep", [False, True], ids=["pad", "keep"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(fc.CASES))
def test_state_tensor_framed(states, name, dtype, keep):
    by_size, framed = states
    (w, h), (ow, oh), _, _, _ = fc.CASES[name]
    st, _ = by_size[(w, h)]
    rc = fc.rects(name)
    bgr = dtype == ref.F16
    scale, bias = ref.EDGES if dtype == ref.F16 else ref.IMAGENET
    stride_h = ow + 3
    stride_c = oh * stride_h + 5
    t = h263mi.make_tensor_out(ow, oh, dtype, scale, bias, bgr=bgr, stride_h=stride_h, stride_c=stride_c)
    n_elem = 1 + h263mi.tensor_extent(1, t) // ref.ELT[dtype] + 7
    out = np.full(n_elem, _sentinel(dtype), ref.BITS_DTYPE[dtype])
    st.render_tensor_framed_into(7, t, _framing(name, keep), out[1:])
    want = np.full(n_elem, _sentinel(dtype), ref.BITS_DTYPE[dtype])
    pl = ref.planes(framed[name], dtype, scale, bias, bgr)
    mask = fref.inside(rc, oh, ow)
    for p in range(3):
        for y in range(oh):
            at = 1 + p * stride_c + y * stride_h
            sel = mask[y] if keep else np.ones(ow, bool)
            want[at:at + ow][sel] = pl[p, y][sel]
    _same(out, want, name)


def test_state_stretch_and_whole_window_are_the_plain_calls(states):
    by_size, _ = states
    st, full = by_size[fc.QCIF]
    w, h = fc.QCIF
    ow, oh = 130, 41
    plain = st.render_rgba_resize(7, ow, oh)
    _same(plain, rgba_resize_ref.resize(full, w, h, ow, oh), "plain")
    for f in (h263mi.make_framing(fref.STRETCH, pad=PAD), h263mi.make_framing(fref.WINDOW, src=(0, 0, w, h), dst=(0, 0, ow, oh)), None):
        _same(st.render_rgba_resize_framed(7, f, ow, oh), plain, "stretch rgba")
    t = h263mi.make_tensor_out(ow, oh, ref.BF16, *ref.IMAGENET)
    plain_t = st.render_tensor(7, t).view(np.uint16)
    out = np.zeros(3 * oh * ow, np.uint16)
    st.render_tensor_framed_into(7, t, h263mi.make_framing(fref.STRETCH, pad=PAD, keep_outside=True), out)
    _same(out, plain_t, "stretch tensor")
    # a refused framing: nothing is written
    out = np.full(4 * ow * oh, SENTINEL, np.uint8)
    with pytest.raises(h263mi.H263Error) as e:
        st.render_rgba_resize_framed_into(7, out, h263mi.make_framing(fref.WINDOW, src=(0, 0, w + 1, h), dst=(0, 0, ow, oh)), ow, oh)
    assert e.value.code == h263mi.ERR_INVALID_ARGUMENT and (out == SENTINEL).all()


# ---------------------------------------------------------------------------------------------
# 2. a batch: LETTERBOX with the grey of detectors, BGR, padded strides, the base one element in, one stream inactive
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def qcif_streams():
    """4 streams of 176 x 144, I then P: device records and the oracle's planes of both pictures"""
    n, w, h = 4, 176, 144
    pics0 = _small_streams(n, w, h, 6100)
    recs0, planes0 = _upload_records(pics0, w, h)
    pics1 = [recgen.inter_picture(w, h, seed=6150 + s, mv_range=30, p_4v=0.2, p_coded=0.5, quant=8) for s in range(n)]
    recs1 = _upload(pics1)
    planes1 = []
    for (m, c), p0 in zip(pics1, planes0):
        rc, p = orc.decode_picture(w, h, m, c, p0)
        assert rc == 0
        planes1.append(p)
    return n, w, h, (recs0, recs1), (planes0, planes1)


def _framed_pics(planes, w, h, strengths, ow, oh, rects, pad):
    return [fref.rgba(_full(p, w, h, s), ow, oh, rects, pad) for p, s in zip(planes, strengths)]


def _tensor_canvas(n_elem, dtype, pics, t, base, stride_n, skip=()):
    want = np.full(n_elem, _sentinel(dtype), ref.BITS_DTYPE[dtype])
    for s, pic in enumerate(pics):
        if s not in skip:
            ref.place(want, ref.planes(pic, dtype, list(t.scale), list(t.bias), bool(t.bgr)), base + s * stride_n, t.stride_c, t.stride_h)
    return want


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_batch_letterbox_bgr_padded_odd_base_one_stream_inactive(qcif_streams, dtype):
    n, w, h, recs, planes = qcif_streams
    ow, oh = 96, 96
    grey = (114, 114, 114)
    f = h263mi.make_framing(fref.LETTERBOX, pad=grey)
    rects = fref.resolve(w, h, ow, oh, fref.LETTERBOX)
    assert rects == ((0, 0, 176, 144), (0, 8, 96, 79))                # rnd(144*96, 176) = 27824 div 352 = 79; (96 - 79) div 2
    got_rc = h263mi.framing_resolve(w, h, ow, oh, f)
    assert (got_rc.src(), got_rc.dst()) == rects
    stride_h = ow + 3
    stride_c = oh * stride_h + 5
    stride_n = 3 * stride_c + 7
    elt = ref.ELT[dtype]
    strengths = np.array([0, 5, 7, 12], np.uint8)
    t = h263mi.make_tensor_out(ow, oh, dtype, *ref.IMAGENET, bgr=True, stride_n=stride_n, stride_c=stride_c, stride_h=stride_h)
    nbytes = h263mi.tensor_extent(n, t)
    b = h263mi.Batch(n, w, h, 0, None)
    b.set_tensor_output_framed(t, f)
    n_elem = 1 + nbytes // elt + 5
    for k, ptype in enumerate((h263mi.PICTURE_I, h263mi.PICTURE_P)):
        if k == 1:
            b.set_active([1, 1, 0, 1])
        c = _canvas(n_elem * elt)
        b.decode(ptype, recs[k][0].ptr, recs[k][1].ptr, recs[k][2].ptr, 0, 0, c.at(elt), None, strengths=strengths)
        b.sync()
        want = _tensor_canvas(n_elem, dtype, _framed_pics(planes[k], w, h, strengths, ow, oh, rects, grey), t, 1, stride_n,
                              skip=(2,) if k else ())
        _same(c.download().view(ref.BITS_DTYPE[dtype]), want, "call %d" % k)
    b.close()


# ---------------------------------------------------------------------------------------------
# 3. a deferred rendering keeps the framing of its request
# ---------------------------------------------------------------------------------------------
def test_pipelined_output_keeps_the_framing_of_its_request():
    n, w, h = 4, 176, 144
    b = h263mi.Batch(n, w, h, 0, None, pipeline_post=True)
    recs = [_upload_records(_small_streams(n, w, h, 6200 + 100 * k), w, h) for k in range(4)]
    # call 1: RGBA letterbox 96 x 96, grey; call 2: bf16 tensor, cover 50 x 70; call 3: RGBA window with keep_outside;
    # call 4: the plain resize
    fa = h263mi.make_framing(fref.LETTERBOX, pad=(114, 114, 114))
    fb = h263mi.make_framing(fref.COVER, pad=PAD)
    name = "qcif_window_odd"
    fcw = _framing(name, keep=True)
    (ow3, oh3) = fc.CASES[name][1]
    tb = h263mi.make_tensor_out(50, 70, ref.BF16, *ref.IMAGENET)
    c1 = _canvas(h263mi.rgba_resize_extent(n, 96, 96))
    c2 = _canvas(h263mi.tensor_extent(n, tb))
    c3 = _canvas(h263mi.rgba_resize_extent(n, ow3, oh3))
    c4 = _canvas(h263mi.rgba_resize_extent(n, 40, 30))
    dec = lambda k, strength, c: b.decode(h263mi.PICTURE_I, recs[k][0][0].ptr, recs[k][0][1].ptr, recs[k][0][2].ptr, 0, strength, c.ptr, None)
    b.set_rgba_resize_framed(fa, 96, 96)
    dec(0, 7, c1)                                                     # deferred
    fa.pad[0] = 1                                                     # (the framing was copied)
    b.set_tensor_output_framed(tb, fb)
    dec(1, 3, c2)                                                     # renders 1
    b.set_rgba_resize_framed(fcw, ow3, oh3)
    dec(2, 5, c3)                                                     # renders 2
    b.set_rgba_resize(40, 30)
    dec(3, 9, c4)                                                     # renders 3
    b.set_rgba_resize_framed(fa, 96, 96)
    b.sync()                                                          # renders 4
    strength = (7, 3, 5, 9)
    pics = lambda k, ow, oh, rects, pad: _framed_pics(recs[k][1], w, h, [strength[k]] * n, ow, oh, rects, pad)
    _same(c1.download(), np.concatenate([p.ravel() for p in pics(0, 96, 96, fref.resolve(w, h, 96, 96, fref.LETTERBOX), (114,) * 3)]),
          "call 1")
    want2 = _tensor_canvas(c2.nbytes // 2, ref.BF16, pics(1, 50, 70, fref.resolve(w, h, 50, 70, fref.COVER), PAD), tb, 0, 3 * 70 * 50)
    _same(c2.download().view(np.uint16), want2, "call 2")
    rects3 = fc.rects(name)
    mask = fref.inside(rects3, oh3, ow3)
    want3 = np.full((n, oh3, ow3, 4), SENTINEL, np.uint8)
    for s, p in enumerate(pics(2, ow3, oh3, rects3, PAD)):
        want3[s][mask] = p[mask]
    _same(c3.download(), want3, "call 3")
    want4 = np.concatenate([rgba_resize_ref.resize(full_rgba(p, w, 9), w, h, 40, 30).ravel() for p in recs[3][1]])
    _same(c4.download(), want4, "call 4")
    b.close()


# ---------------------------------------------------------------------------------------------
# 4. identity routing: a framing that is whole onto whole is the unframed shape, its fused layouts included
# ---------------------------------------------------------------------------------------------
def test_same_aspect_letterbox_is_the_plain_resize_byte_for_byte():
    n, w, h = 2, 352, 288
    recs, planes = _upload_records(_small_streams(n, w, h, 6600), w, h)
    outs = []
    for framed in (False, True):
        b = h263mi.Batch(n, w, h, 0, None)
        if framed:
            b.set_rgba_resize_framed(h263mi.make_framing(fref.LETTERBOX, pad=PAD), 176, 144)
        else:
            b.set_rgba_resize(176, 144)
        c = _canvas(h263mi.rgba_resize_extent(n, 176, 144))
        b.decode(h263mi.PICTURE_I, recs[0].ptr, recs[1].ptr, recs[2].ptr, 0, 5, c.ptr, None)
        b.sync()
        outs.append(c.download())
        b.close()
    _same(outs[1], outs[0], "framed against plain")
    want = np.concatenate([rgba_resize_ref.resize(full_rgba(p, w, 5), w, h, 176, 144).ravel() for p in planes])
    _same(outs[0], want, "plain against the reference")


# ---------------------------------------------------------------------------------------------
# 5. refusals queue nothing, and the shape in force survives them
# ---------------------------------------------------------------------------------------------
def test_refusals_queue_nothing_and_keep_the_shape(qcif_streams):
    n, w, h, recs, planes = qcif_streams
    ow, oh = 96, 96
    good = h263mi.make_framing(fref.LETTERBOX, pad=(114, 114, 114))
    b = h263mi.Batch(n, w, h, 0, None)
    b.set_rgba_resize_framed(good, ow, oh)
    bads = [h263mi.make_framing(4), h263mi.make_framing(fref.WINDOW, src=(0, 0, w + 1, h), dst=(0, 0, ow, oh)),
            h263mi.make_framing(fref.WINDOW, src=(0, 0, w, h), dst=(1, 0, ow, oh)), h263mi.make_framing(fref.COVER, dst=(0, 0, 1, 1))]
    r = h263mi.make_framing(fref.LETTERBOX)
    r.reserved[1] = 1
    k = h263mi.make_framing(fref.LETTERBOX)
    k.keep_outside = 2
    t = h263mi.make_tensor_out(ow, oh, ref.F32)
    for bad in bads + [r, k]:
        with pytest.raises(h263mi.H263Error) as e:
            b.set_rgba_resize_framed(bad, ow, oh)
        assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
        with pytest.raises(h263mi.H263Error) as e:
            b.set_tensor_output_framed(t, bad)
        assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    nbytes = h263mi.rgba_resize_extent(n, ow, oh)
    dec = lambda ptr: b.decode(h263mi.PICTURE_I, recs[0][0].ptr, recs[0][1].ptr, recs[0][2].ptr, 0, 5, ptr, None)
    short = _canvas(nbytes - 1)                                       # one byte short on a checked batch
    with pytest.raises(h263mi.H263Error) as e:
        dec(short.ptr)
    assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    assert not any(b.stream_has_picture(s) for s in range(n))        # no stream advanced
    b.sync()
    assert (short.download() == SENTINEL).all()
    okc = _canvas(nbytes)
    dec(okc.ptr)
    b.sync()
    rects = fref.resolve(w, h, ow, oh, fref.LETTERBOX)
    want = np.concatenate([p.ravel() for p in _framed_pics(planes[0], w, h, [5] * n, ow, oh, rects, (114,) * 3)])
    _same(okc.download(), want, "after the refusals")
    b.close()


# ---------------------------------------------------------------------------------------------
# 6. a mixed-size set: every size keeps its own aspect ratio inside ONE [4, 3, 64, 96] tensor
# ---------------------------------------------------------------------------------------------
class _Part:
    """a part of a device buffer, as MixedBatch.decode_next_pictures takes it"""

    def __init__(self, buf, offset, nbytes):
        self.ptr, self.nbytes = buf.at(offset), nbytes


@pytest.mark.parametrize("dtype", [ref.F32, ref.BF16], ids=["f32", "bf16"])
def test_mixed_set_letterboxed_into_one_tensor(dtype):
    import sorenson_enc as enc
    from test_bitstream_e2e import make_codable
    q, strength = 6, 5
    sizes = [(176, 144), (352, 288), (320, 240), (128, 96)]
    n, ow, oh, elt = len(sizes), 96, 64, ref.ELT[dtype]
    grey = (114, 114, 114)
    f = h263mi.make_framing(fref.LETTERBOX, pad=grey)
    t = h263mi.make_tensor_out(ow, oh, dtype, *ref.IMAGENET)
    one = h263mi.tensor_extent(1, t)
    m = h263mi.MixedBatch(n)
    for bad in (h263mi.make_framing(fref.WINDOW, src=(0, 0, 8, 8), dst=(0, 0, 8, 8)), h263mi.make_framing(5)):
        with pytest.raises(h263mi.H263Error) as e:
            m.set_tensor_output_framed(t, bad)
        assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
        with pytest.raises(h263mi.H263Error) as e:
            m.set_rgba_resize_framed(bad, ow, oh)
        assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    with pytest.raises(h263mi.H263Error) as e:                        # no picture yet
        m.stream_framing(0)
    assert e.value.code == h263mi.ERR_NO_PICTURE
    m.set_tensor_output_framed(t, f)
    buf = _canvas(n * one)
    datas, wants, rects = [], [], []
    for s, (w, h) in enumerate(sizes):
        mbs, co = recgen.intra_picture(w, h, seed=7000 + s, max_level=60)
        mbs = make_codable(mbs, q, s, 0)
        datas.append(enc.encode_picture(w, h, 0, q, mbs, co, temporal_reference=0))
        rc, planes = orc.decode_picture(w, h, mbs, co, None)
        assert rc == 0
        rects.append(fref.resolve(w, h, ow, oh, fref.LETTERBOX))
        wants.append(fref.rgba(_full(planes, w, h, strength), ow, oh, rects[-1], grey))
    parts = [_Part(buf, s * one, one) for s in range(n)]
    used, rcs, _ = m.decode_next_pictures(datas, n_threads=2, strength=strength, rgba=parts)
    assert not any(m.sync()) and list(rcs) == [0] * n
    for s in range(n):
        got = m.stream_framing(s)
        assert (got.src(), got.dst()) == rects[s], (s, got.src(), got.dst(), rects[s])
    # the 11:9 and the 4:3 classes keep their own aspect ratios
    assert rects[0][1] == rects[1][1] == (9, 0, 78, 64) and rects[2][1] == rects[3][1] == (5, 0, 85, 64)
    _same(buf.download().view(ref.BITS_DTYPE[dtype]), _tensor_canvas(n * one // elt, dtype, wants, t, 0, 3 * oh * ow), "the tensor")
    # what is really allocated counts: the full-size pictures of every class and its own span tables
    with_tensor = m.frame_store_bytes()
    m.set_tensor_output(None)
    bare = m.frame_store_bytes()
    scratch = 4 * sum(w * h for w, h in sizes) + 16 * sum(r[1][2] + r[1][3] for r in rects)
    assert with_tensor - bare == scratch
    m.set_tensor_output(t)
    assert m.frame_store_bytes() - bare == 4 * sum(w * h for w, h in sizes) + 16 * n * (ow + oh)
    m.set_tensor_output_framed(t, f)
    assert m.frame_store_bytes() == with_tensor
    m.set_tensor_output(None)
    assert m.frame_store_bytes() == bare
    m.close()
